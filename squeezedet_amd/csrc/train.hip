// Training-path kernels for gfx950 (float32 storage, the reference's training dtype):
//   conv backward-data   -- the forward conv kernel run on the 180-degree-rotated, in/out-swapped
//                           kernel (stride-1 SAME convs: every trainable conv of SqueezeDet);
//   conv backward-filter -- split-K GEMM over pixels on the exact-f32 MFMA, deterministic two-pass
//                           reduction (no atomics), + bias gradient;
//   ReLU / max-pool / dropout backward, the residual add, the concat copy, the sum of the mask.
// (The loss lives in loss.hip, the optimizer in optim.hip.)
// Compiled with -ffp-contract=off (bn_fold.h's expressions; convert_scale shares scaled_to with the loss's float16 stores).
#include <math.h>

#include "bn_fold.h"
#include "conv_common.h"
#include "item_table.h"
#include "train_common.h"

namespace sqdet {

// ------------------------------------------------------------------ backward-data weight packing
// The kernel of the backward-data conv, packed in the forward fragment order for a [k,k,cout,cin] kernel (conv_common.h).
template <typename T>
__global__ void pack_bwd_data_kernel(const float* __restrict__ w, T* __restrict__ out, int k, int cin, int cout,
                                     int nchunk, int nt, size_t total) {
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    float v;
    pack_fetch_bwd(w, pack_index<T>(idx, nt, nchunk, k * k), k, cin, cout, v);
    out[idx] = (T)v;
  }
}

// ------------------------------------------------------------------ packing MANY kernels in one launch
// A training step re-packs every trainable conv kernel twice (forward fragment order + the backward-data conv's order) after
// the optimizer has changed it: 62 launches of ~4.7 us in SqueezeDet's step -- 0.29 ms of 3.5.  One launch walks a table
// (item_table.h).
struct PackItem {
  const float* w;        // HWIO float32 [k,k,cin,cout]
  void* out;             // packed buffer
  int k, cin, cout;
  int taps, kdim, nchunk, nt;   // of the conv that will READ the packed kernel (forward: cin -> cout; backward-data: cout -> cin)
  int bwd;               // 0 forward order, 1 backward-data order
  unsigned long long total;
  unsigned first_block, nblocks;
  // gamma != NULL: the kernel of a _conv_bn_layer -- what is packed is the FOLDED kernel W[..., c] * bn_fold_scale(c), and the
  // item's first workgroup also writes the folded bias b_folded (when not NULL)
  const float *gamma, *var, *beta, *mean, *cbias;
  float* b_folded;
  float eps;
};

template <typename T>
__global__ __launch_bounds__(256) void pack_many_kernel(const PackItem* __restrict__ items, int nitems) {
  const PackItem p = item_of_block<PackItem, &PackItem::first_block>(items, nitems, blockIdx.x);
  const float* __restrict__ w = p.w;
  T* __restrict__ out = reinterpret_cast<T*>(p.out);
  for (size_t idx = (size_t)(blockIdx.x - p.first_block) * 256 + threadIdx.x; idx < p.total; idx += (size_t)p.nblocks * 256) {
    const PackIdx x = pack_index<T>(idx, p.nt, p.nchunk, p.taps);
    float v;
    const bool in = p.bwd ? pack_fetch_bwd(w, x, p.k, p.cin, p.cout, v) : pack_fetch_fwd(w, x, p.kdim, p.cout, v);
    if (p.gamma && in) {
      const int oc = p.bwd ? x.ci : x.co;       // the ORIGINAL output channel of the element (the batch-norm channel)
      v = v * bn_fold_scale(p.gamma[oc], p.var[oc], p.eps);
    }
    out[idx] = (T)v;
  }
  if (p.gamma && p.b_folded && blockIdx.x == p.first_block) {
    for (int c = threadIdx.x; c < p.cout; c += 256)
      p.b_folded[c] = bn_fold_bias(p.cbias, p.mean, p.beta, c, bn_fold_scale(p.gamma[c], p.var[c], p.eps));
  }
}

// (conv backward-filter lives in wgrad.hip)
// out[e] = sum_z partial[z][e]  (+ decay * w[e] when w != NULL), z ascending: deterministic.
__global__ void slab_reduce_kernel(const float* __restrict__ partial, float* __restrict__ out, const float* __restrict__ w,
                                   float decay, size_t count, int nslabs) {
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < count; e += (size_t)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int z = 0; z < nslabs; ++z) s += partial[(size_t)z * count + e];
    if (w) s += decay * w[e];
    out[e] = s;
  }
}

// ------------------------------------------------------------------ elementwise backward ops
// (float32, or float16 for mixed-precision training; 16-byte vectors of EV elements)
template <typename T> struct Vec16 { typedef T type __attribute__((ext_vector_type(16 / sizeof(T)))); };

template <typename T>
__global__ void relu_bwd_kernel(const T* __restrict__ y, T* __restrict__ dy, size_t nv) {
  typedef typename Vec16<T>::type V;
  constexpr int EV = 16 / sizeof(T);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x) {
    const V v = reinterpret_cast<const V*>(y)[i];
    V g = reinterpret_cast<V*>(dy)[i];
#pragma unroll
    for (int e = 0; e < EV; ++e) g[e] = v[e] > (T)0 ? g[e] : (T)0;
    reinterpret_cast<V*>(dy)[i] = g;
  }
}

// y = x * mask * scale  (tf.nn.dropout forward with mask = floor(keep_prob + U), scale = 1/keep_prob; and its backward)
template <typename T>
__global__ void scale_mask_kernel(const T* __restrict__ x, const T* __restrict__ mask, T* __restrict__ y, float scale, size_t nv) {
  typedef typename Vec16<T>::type V;
  constexpr int EV = 16 / sizeof(T);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x) {
    const V v = reinterpret_cast<const V*>(x)[i];
    const V m = reinterpret_cast<const V*>(mask)[i];
    V o;
#pragma unroll
    for (int e = 0; e < EV; ++e) o[e] = (T)((float)v[e] * (float)m[e] * scale);
    reinterpret_cast<V*>(y)[i] = o;
  }
}

// the same followed by the ReLU backward of the tensor x is the gradient of (relu_of = that ReLU's output): the dropout
// backward in front of conv12 and fire11's ReLU backward in one pass
template <typename T>
__global__ void scale_mask_relu_kernel(const T* __restrict__ x, const T* __restrict__ mask, const T* __restrict__ relu_of,
                                       T* __restrict__ y, float scale, size_t nv) {
  typedef typename Vec16<T>::type V;
  constexpr int EV = 16 / sizeof(T);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x) {
    const V v = reinterpret_cast<const V*>(x)[i];
    const V m = reinterpret_cast<const V*>(mask)[i];
    const V r = reinterpret_cast<const V*>(relu_of)[i];
    V o;
#pragma unroll
    for (int e = 0; e < EV; ++e) {
      const T t = (T)((float)v[e] * (float)m[e] * scale);
      o[e] = r[e] > (T)0 ? t : (T)0;
    }
    reinterpret_cast<V*>(y)[i] = o;
  }
}

// dst = (D)(src * scale): the float16 <-> float32 hand-offs of mixed-precision training (preds -> loss, dpreds * loss_scale)
template <typename S, typename D>
__global__ void convert_scale_kernel(const S* __restrict__ src, D* __restrict__ dst, float scale, size_t n4) {
  typedef S SV __attribute__((ext_vector_type(4)));
  typedef D DV __attribute__((ext_vector_type(4)));
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) {
    const SV v = reinterpret_cast<const SV*>(src)[i];
    DV o;
#pragma unroll
    for (int e = 0; e < 4; ++e) o[e] = scaled_to<D>((float)v[e], scale);
    reinterpret_cast<DV*>(dst)[i] = o;
  }
}

// max-pool backward for the nets' 3x3 / stride-2 pools, gather form (deterministic, no atomics).  In padded
// coordinates (u, v) = (iy + pt, ix + pl) window (oy, ox) covers u in [2oy, 2oy+2]; a thread owns the 2x2 cell block
// u in {2a, 2a+1}, v in {2b, 2b+1}, which only the four windows (a-1..a, b-1..b) touch: it finds each window's FIRST
// maximum (row-major scan, tf.nn.max_pool's argmax) once and hands dy to whichever of its cells that is -- 36 loads
// per block instead of the 81 of a per-cell search.  Windows are visited (a,b), (a,b-1), (a-1,b), (a-1,b-1): the
// summation order of the generic kernel below, so the two agree bitwise.
template <typename T>
__global__ void maxpool3s2_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx,
                                      int N, int H, int W, int C, int pt, int pl, int Ho, int Wo, int BA, int BB, int relu) {
  typedef typename Vec16<T>::type V;
  constexpr int EV = 16 / sizeof(T);
  const int cvn = C / EV;
  const size_t total = (size_t)N * BA * BB * cvn;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int cv = (int)(idx % cvn);
    size_t p = idx / cvn;
    const int b = (int)(p % BB); p /= BB;
    const int a = (int)(p % BA);
    const int n = (int)(p / BA);
    float g[4][EV];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < EV; ++e) g[q][e] = 0.f;
#pragma unroll
    for (int wy = 0; wy < 2; ++wy)
#pragma unroll
      for (int wx = 0; wx < 2; ++wx) {
        const int oy = a - wy, ox = b - wx;
        if (oy < 0 || oy >= Ho || ox < 0 || ox >= Wo) continue;
        float best[EV];
        int bpos[EV];   // 3 * (row in window) + (col in window)
#pragma unroll
        for (int e = 0; e < EV; ++e) { best[e] = -INFINITY; bpos[e] = -1; }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          const int yy = 2 * oy - pt + r;
          if (yy < 0 || yy >= H) continue;
#pragma unroll
          for (int c = 0; c < 3; ++c) {
            const int xx = 2 * ox - pl + c;
            if (xx < 0 || xx >= W) continue;
            const V v = *reinterpret_cast<const V*>(x + ((((size_t)n * H + yy) * W + xx) * C + cv * EV));
#pragma unroll
            for (int e = 0; e < EV; ++e) {
              // the first valid cell NAMES the window until a cell wins the strict comparison against -inf (a NaN never wins): a
              // window of -inf / NaN cells still routes its gradient, to that cell -- maxpool3_idx_kernel's rule, bit for bit
              if (bpos[e] < 0) bpos[e] = 3 * r + c;
              if ((float)v[e] > best[e]) { best[e] = (float)v[e]; bpos[e] = 3 * r + c; }
            }
          }
        }
        const V d = *reinterpret_cast<const V*>(dy + ((((size_t)n * Ho + oy) * Wo + ox) * C + cv * EV));
        // this block's cells inside window (oy, ox): window rows 2*wy + {0,1}, cols 2*wx + {0,1} (those < 3)
#pragma unroll
        for (int du = 0; du < 2; ++du)
#pragma unroll
          for (int dv = 0; dv < 2; ++dv) {
            const int r = 2 * wy + du, c = 2 * wx + dv;
            if (r > 2 || c > 2) continue;
#pragma unroll
            for (int e = 0; e < EV; ++e)
              if (bpos[e] == 3 * r + c) g[du * 2 + dv][e] += (float)d[e];
          }
      }
#pragma unroll
    for (int du = 0; du < 2; ++du)
#pragma unroll
      for (int dv = 0; dv < 2; ++dv) {
        const int iy = 2 * a + du - pt, ix = 2 * b + dv - pl;
        if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
        V o;
#pragma unroll
        for (int e = 0; e < EV; ++e) o[e] = (T)g[du * 2 + dv][e];
        if (relu) {   // x is a ReLU output: the ReLU backward of the layer below, here instead of a pass of its own
          const V xv = *reinterpret_cast<const V*>(x + ((((size_t)n * H + iy) * W + ix) * C + cv * EV));
#pragma unroll
          for (int e = 0; e < EV; ++e) o[e] = xv[e] > (T)0 ? o[e] : (T)0;
        }
        *reinterpret_cast<V*>(dx + ((((size_t)n * H + iy) * W + ix) * C + cv * EV)) = o;
      }
  }
}

// The same from the window index the training forward recorded (pool.hip maxpool3_idx_kernel): per 2x2 cell block four
// windows' idx (one byte per channel) + dy -- and, for the fused ReLU backward, the POOLED y: a cell that receives anything is
// the argmax of a window whose output y equals the cell's x, so (x > 0) == (y > 0) for every contribution it sums -- instead
// of 25 full-resolution 16-byte cells of x.  Same window order and the same sums as maxpool3s2_bwd_kernel: bitwise equal.
template <typename T>
__global__ void maxpool3s2_bwd_idx_kernel(const unsigned char* __restrict__ widx, const T* __restrict__ y,
                                          const T* __restrict__ dy, T* __restrict__ dx, int N, int H, int W, int C, int pt,
                                          int pl, int Ho, int Wo, int BA, int BB, int relu) {
  typedef typename Vec16<T>::type V;
  constexpr int EV = 16 / sizeof(T);
  const int cvn = C / EV;
  const size_t total = (size_t)N * BA * BB * cvn;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int cv = (int)(idx % cvn);
    size_t p = idx / cvn;
    const int b = (int)(p % BB); p /= BB;
    const int a = (int)(p % BA);
    const int n = (int)(p / BA);
    float g[4][EV];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < EV; ++e) g[q][e] = 0.f;
#pragma unroll
    for (int wy = 0; wy < 2; ++wy)
#pragma unroll
      for (int wx = 0; wx < 2; ++wx) {
        const int oy = a - wy, ox = b - wx;
        if (oy < 0 || oy >= Ho || ox < 0 || ox >= Wo) continue;
        const size_t o = (((size_t)n * Ho + oy) * Wo + ox) * C + cv * EV;
        unsigned char bp[EV];
        if constexpr (EV == 8) {
          typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
          const u32x2 w2 = *reinterpret_cast<const u32x2*>(widx + o);
#pragma unroll
          for (int e = 0; e < 8; ++e) bp[e] = (unsigned char)(w2[e >> 2] >> (8 * (e & 3)));
        } else {
          const unsigned int w1 = *reinterpret_cast<const unsigned int*>(widx + o);
#pragma unroll
          for (int e = 0; e < 4; ++e) bp[e] = (unsigned char)(w1 >> (8 * e));
        }
        V d = *reinterpret_cast<const V*>(dy + o);
        if (relu) {
          const V yv = *reinterpret_cast<const V*>(y + o);
#pragma unroll
          for (int e = 0; e < EV; ++e) d[e] = yv[e] > (T)0 ? d[e] : (T)0;
        }
#pragma unroll
        for (int du = 0; du < 2; ++du)
#pragma unroll
          for (int dv = 0; dv < 2; ++dv) {
            const int r = 2 * wy + du, c = 2 * wx + dv;
            if (r > 2 || c > 2) continue;
#pragma unroll
            for (int e = 0; e < EV; ++e)
              if (bp[e] == 3 * r + c) g[du * 2 + dv][e] += (float)d[e];
          }
      }
#pragma unroll
    for (int du = 0; du < 2; ++du)
#pragma unroll
      for (int dv = 0; dv < 2; ++dv) {
        const int iy = 2 * a + du - pt, ix = 2 * b + dv - pl;
        if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
        V o;
#pragma unroll
        for (int e = 0; e < EV; ++e) o[e] = (T)g[du * 2 + dv][e];
        *reinterpret_cast<V*>(dx + ((((size_t)n * H + iy) * W + ix) * C + cv * EV)) = o;
      }
  }
}

// The 2x2 / stride-2 form from the window index (pool.hip maxpool2_idx_kernel): the windows do not overlap, so one thread per
// output vector writes its whole 2x2 block of dx -- dy at the winner, zero elsewhere; no gather, no accumulation.  Threads run
// over the ceil((H + pt) / 2) x ceil((W + pl) / 2) blocks: a block past Ho / Wo (VALID with an odd H or W: the last row or
// column belongs to no window) is written as zeros, so every dx cell is written.  The winner's value is (T)(0.f + (float)dy),
// the sum maxpool_bwd_kernel forms (-0 -> +0): bitwise sqdet_maxpool_nhwc_bwd / _bwd_relu.  relu: (y > 0) at the winner, the
// pooled value being the winner's x.
template <typename T>
__global__ void maxpool2s2_bwd_idx_kernel(const unsigned char* __restrict__ widx, const T* __restrict__ y,
                                          const T* __restrict__ dy, T* __restrict__ dx, int N, int H, int W, int C, int pt,
                                          int pl, int Ho, int Wo, int BA, int BB, int relu) {
  typedef typename Vec16<T>::type V;
  constexpr int EV = 16 / sizeof(T);
  const int cvn = C / EV;
  const size_t total = (size_t)N * BA * BB * cvn;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int cv = (int)(idx % cvn);
    size_t p = idx / cvn;
    const int b = (int)(p % BB); p /= BB;
    const int a = (int)(p % BA);
    const int n = (int)(p / BA);
    V o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int e = 0; e < EV; ++e) o[q][e] = (T)0.f;
    if (a < Ho && b < Wo) {
      const size_t oo = (((size_t)n * Ho + a) * Wo + b) * C + cv * EV;
      unsigned char bp[EV];
      if constexpr (EV == 8) {
        typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
        const u32x2 w2 = *reinterpret_cast<const u32x2*>(widx + oo);
#pragma unroll
        for (int e = 0; e < 8; ++e) bp[e] = (unsigned char)(w2[e >> 2] >> (8 * (e & 3)));
      } else {
        const unsigned int w1 = *reinterpret_cast<const unsigned int*>(widx + oo);
#pragma unroll
        for (int e = 0; e < 4; ++e) bp[e] = (unsigned char)(w1 >> (8 * e));
      }
      const V d = *reinterpret_cast<const V*>(dy + oo);
      V yv;
      if (relu) yv = *reinterpret_cast<const V*>(y + oo);
#pragma unroll
      for (int e = 0; e < EV; ++e) {
        const T gv = (T)(0.f + (float)d[e]);
        const T v = relu && !(yv[e] > (T)0) ? (T)0.f : gv;
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q][e] = bp[e] == q ? v : o[q][e];
      }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int iy = 2 * a + (q >> 1) - pt, ix = 2 * b + (q & 1) - pl;
      if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
      *reinterpret_cast<V*>(dx + ((((size_t)n * H + iy) * W + ix) * C + cv * EV)) = o[q];
    }
  }
}

// max-pool backward, generic gather form (deterministic): an input cell receives dy of every window whose
// FIRST maximum (row-major scan, as tf.nn.max_pool's argmax) it is.
template <typename T>
__global__ void maxpool_bwd_kernel(const T* __restrict__ x, const T* __restrict__ dy, T* __restrict__ dx,
                                   int N, int H, int W, int C, int k, int stride, int pt, int pl, int Ho, int Wo, int relu) {
  typedef typename Vec16<T>::type V;
  constexpr int EV = 16 / sizeof(T);
  const int cvn = C / EV;
  const size_t total = (size_t)N * H * W * cvn;
  for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    const int cv = (int)(idx % cvn);
    size_t p = idx / cvn;
    const int ix = (int)(p % W); p /= W;
    const int iy = (int)(p % H);
    const int n = (int)(p / H);
    float g[EV];
#pragma unroll
    for (int e = 0; e < EV; ++e) g[e] = 0.f;
    // windows (oy, ox) containing (iy, ix): oy*stride - pt <= iy <= oy*stride - pt + k - 1
    const int oy_hi = (iy + pt) / stride, ox_hi = (ix + pl) / stride;
    for (int oy = oy_hi; oy >= 0 && oy * stride - pt + k - 1 >= iy; --oy) {
      if (oy >= Ho) continue;
      for (int ox = ox_hi; ox >= 0 && ox * stride - pl + k - 1 >= ix; --ox) {
        if (ox >= Wo) continue;
        // first argmax of the window, per channel: position code yy * W + xx
        float best[EV];
        int bpos[EV];
#pragma unroll
        for (int e = 0; e < EV; ++e) { best[e] = -INFINITY; bpos[e] = -1; }
        for (int dy_ = 0; dy_ < k; ++dy_) {
          const int yy = oy * stride - pt + dy_;
          if (yy < 0 || yy >= H) continue;
          for (int dx_ = 0; dx_ < k; ++dx_) {
            const int xx = ox * stride - pl + dx_;
            if (xx < 0 || xx >= W) continue;
            const V v = *reinterpret_cast<const V*>(x + ((((size_t)n * H + yy) * W + xx) * C + cv * EV));
#pragma unroll
            for (int e = 0; e < EV; ++e) {
              if (bpos[e] < 0) bpos[e] = yy * W + xx;      // (the first valid cell names a window nothing wins: all -inf / NaN)
              if ((float)v[e] > best[e]) { best[e] = (float)v[e]; bpos[e] = yy * W + xx; }
            }
          }
        }
        const V d = *reinterpret_cast<const V*>(dy + ((((size_t)n * Ho + oy) * Wo + ox) * C + cv * EV));
#pragma unroll
        for (int e = 0; e < EV; ++e)
          if (bpos[e] == iy * W + ix) g[e] += (float)d[e];
      }
    }
    V o;
#pragma unroll
    for (int e = 0; e < EV; ++e) o[e] = (T)g[e];
    if (relu) {
      const V xv = *reinterpret_cast<const V*>(x + idx * EV);
#pragma unroll
      for (int e = 0; e < EV; ++e) o[e] = xv[e] > (T)0 ? o[e] : (T)0;
    }
    *reinterpret_cast<V*>(dx + idx * EV) = o;
  }
}

// out[0] = sum of x[0..n) in a fixed order (one 1024-thread workgroup: per-thread strided partial sums over 16-byte
// vectors with four independent accumulators -- the first version walked 1300 dependent 4-byte loads per thread, 300 us of a
// 12 ms training step --, then a tree over LDS): num_objects = sum(input_mask), nn_skeleton.py:180, without a device -> host
// round trip
__global__ __launch_bounds__(1024) void sum_f32_kernel(const float* __restrict__ x, size_t n, float* __restrict__ out) {
  __shared__ float red[1024];
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0;
  const size_t nv = vec ? n / 4 : 0;
  size_t i = threadIdx.x;
  for (; i + 7 * 1024 < nv; i += 8 * 1024) {      // eight loads in flight (one at a time, 337 k floats took 36 us); same add order
    f32x4 v[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) v[u] = reinterpret_cast<const f32x4*>(x)[i + u * 1024];
#pragma unroll
    for (int u = 0; u < 8; ++u) { s0 += v[u][0]; s1 += v[u][1]; s2 += v[u][2]; s3 += v[u][3]; }
  }
  for (; i < nv; i += 1024) {
    const f32x4 v = reinterpret_cast<const f32x4*>(x)[i];
    s0 += v[0]; s1 += v[1]; s2 += v[2]; s3 += v[3];
  }
  for (size_t i = nv * 4 + threadIdx.x; i < n; i += 1024) s0 += x[i];
  red[threadIdx.x] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  for (int w = 512; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[0] = red[0];
}

// y = max(a + b, 0) (tf.nn.relu(shortcut + branch), resnet50_convDet.py:55) -- the residual add where the producing conv
// could not take it in its epilogue; 16-byte vectors
template <typename T>
__global__ void add_relu_kernel(const T* __restrict__ a, const T* __restrict__ b, T* __restrict__ y, size_t nv) {
  typedef typename Vec16<T>::type V;
  constexpr int EV = 16 / sizeof(T);
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x) {
    const V va = reinterpret_cast<const V*>(a)[i], vb = reinterpret_cast<const V*>(b)[i];
    V r;
#pragma unroll
    for (int e = 0; e < EV; ++e) { const float t = (float)va[e] + (float)vb[e]; r[e] = (T)(t > 0.f ? t : 0.f); }
    reinterpret_cast<V*>(y)[i] = r;
  }
}

// y[p, coff .. coff + c) = x[p, 0 .. c): one input of tf.concat(axis=3) (nets/squeezeDet.py:106); 16-byte vectors
template <typename T>
__global__ void copy_channels_kernel(const T* __restrict__ x, T* __restrict__ y, size_t pixels, int cv, int cstride_v, int coff_v) {
  typedef typename Vec16<T>::type V;
  const size_t total = pixels * (size_t)cv;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t p = i / cv;
    const int c = (int)(i - p * cv);
    reinterpret_cast<V*>(y)[p * cstride_v + coff_v + c] = reinterpret_cast<const V*>(x)[i];
  }
}

// mask[i] = floor(keep_prob + u_i), u_i uniform in [0,1): tf.nn.dropout's keep mask (nets/squeezeDet.py:74).  Counter-based
// generator (one 64-bit mix of (seed, i) per element -- splitmix64), so the mask depends on (seed, index) only.
template <typename T>
__global__ void dropout_mask_kernel(T* __restrict__ mask, size_t n, float keep_prob, unsigned long long seed) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(i + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const float u = (float)(z >> 40) * (1.0f / 16777216.0f);   // 24 random bits -> [0, 1)
    // keep_prob = 1 and the top draw u = 1 - 2^-24: the float32 sum 2 - 2^-24 is a tie that rounds to 2.0 -- a keep mask holds 0 or 1
    mask[i] = (T)fminf(floorf(keep_prob + u), 1.0f);
  }
}

static int grid_for(size_t n, int cap = 4096) {
  size_t b = (n + 255) / 256;
  if (b > (size_t)cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

}  // namespace sqdet

using namespace sqdet;

extern "C" int sqdet_conv_pack_weights_bwd_data(const float* w_hwio_f32, void* packed, int k, int cin, int cout,
                                                int dtype, sqdet_stream_t stream) {
  SQDET_REQUIRE(w_hwio_f32 && packed && k > 0 && cin > 0 && cout > 0, "pack_weights_bwd_data: bad arguments");
  SQDET_REQUIRE(dtype == SQDET_F16 || dtype == SQDET_F32, "pack_weights_bwd_data: bad dtype");
  const ConvGeom g = conv_geom(k, cout, cin, dtype);   // the dgrad conv: cout -> cin channels
  SQDET_UNSUPPORTED(g.gather, "pack_weights_bwd_data: cout %d must be a multiple of %d", cout, g.kg);
  const size_t total = (size_t)g.ngroups * g.steps * g.nt * 64 * g.kg;
  if (dtype == SQDET_F16)
    hipLaunchKernelGGL(pack_bwd_data_kernel<f16>, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), w_hwio_f32,
                       (f16*)packed, k, cin, cout, g.nchunk, g.nt, total);
  else
    hipLaunchKernelGGL(pack_bwd_data_kernel<float>, dim3(grid_for(total)), dim3(256), 0, as_stream(stream), w_hwio_f32,
                       (float*)packed, k, cin, cout, g.nchunk, g.nt, total);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

extern "C" size_t sqdet_conv_pack_many_table_bytes(int nitems) { return (size_t)(nitems > 0 ? nitems : 0) * sizeof(sqdet::PackItem); }

extern "C" int sqdet_conv_pack_many_prepare_bn(const float* const* w_hwio_f32, void* const* packed, const int* k, const int* cin,
                                               const int* cout, const int* bwd_data, const float* const* gamma,
                                               const float* const* beta, const float* const* mean, const float* const* var,
                                               const float* const* conv_bias, float* const* b_folded, float eps, int nitems,
                                               int dtype, void* table_host, int* total_blocks) {
  SQDET_REQUIRE(w_hwio_f32 && packed && k && cin && cout && bwd_data && table_host && total_blocks && nitems > 0, "pack_many_prepare: bad arguments");
  SQDET_REQUIRE(dtype == SQDET_F16 || dtype == SQDET_F32, "pack_many_prepare: bad dtype");
  SQDET_REQUIRE(!gamma || (beta && mean && var && conv_bias && b_folded && eps >= 0.f), "pack_many_prepare: incomplete batch-norm arrays");
  sqdet::PackItem* t = reinterpret_cast<sqdet::PackItem*>(table_host);
  sqdet::BlockCursor blocks;
  for (int i = 0; i < nitems; ++i) {
    SQDET_REQUIRE(w_hwio_f32[i] && packed[i] && k[i] > 0 && cin[i] > 0 && cout[i] > 0, "pack_many_prepare: bad item %d", i);
    const ConvGeom g = bwd_data[i] ? conv_geom(k[i], cout[i], cin[i], dtype) : conv_geom(k[i], cin[i], cout[i], dtype);
    SQDET_UNSUPPORTED(bwd_data[i] && g.gather, "pack_many_prepare: item %d: cout %d must be a multiple of %d for the backward-data order", i, cout[i], g.kg);
    sqdet::PackItem& p = t[i];
    p.w = w_hwio_f32[i]; p.out = packed[i]; p.k = k[i]; p.cin = cin[i]; p.cout = cout[i];
    p.taps = g.taps; p.kdim = g.kdim; p.nchunk = g.nchunk; p.nt = g.nt; p.bwd = bwd_data[i] ? 1 : 0;
    p.total = (unsigned long long)g.ngroups * g.steps * g.nt * 64 * g.kg;
    const unsigned long long nb = (p.total + 255) / 256;
    p.nblocks = nb > 256 ? 256u : (unsigned)nb;
    p.first_block = blocks.take(p.nblocks);
    p.gamma = p.var = p.beta = p.mean = p.cbias = nullptr; p.b_folded = nullptr; p.eps = eps;
    if (gamma && gamma[i]) {
      SQDET_REQUIRE(beta[i] && mean[i] && var[i], "pack_many_prepare: item %d: gamma without beta / mean / var", i);
      p.gamma = gamma[i]; p.beta = beta[i]; p.mean = mean[i]; p.var = var[i]; p.cbias = conv_bias[i]; p.b_folded = b_folded[i];
    }
  }
  *total_blocks = (int)blocks.total;
  return SQDET_OK;
}

extern "C" int sqdet_conv_pack_many_prepare(const float* const* w_hwio_f32, void* const* packed, const int* k, const int* cin,
                                            const int* cout, const int* bwd_data, int nitems, int dtype, void* table_host,
                                            int* total_blocks) {
  return sqdet_conv_pack_many_prepare_bn(w_hwio_f32, packed, k, cin, cout, bwd_data, nullptr, nullptr, nullptr, nullptr, nullptr,
                                         nullptr, 0.f, nitems, dtype, table_host, total_blocks);
}

extern "C" int sqdet_conv_pack_many(const void* table_dev, int nitems, int total_blocks, int dtype, sqdet_stream_t stream) {
  SQDET_REQUIRE(table_dev && nitems > 0 && total_blocks > 0, "pack_many: bad arguments");
  SQDET_REQUIRE(dtype == SQDET_F16 || dtype == SQDET_F32, "pack_many: bad dtype");
  const sqdet::PackItem* t = reinterpret_cast<const sqdet::PackItem*>(table_dev);
  if (dtype == SQDET_F16) hipLaunchKernelGGL(sqdet::pack_many_kernel<f16>, dim3(total_blocks), dim3(256), 0, as_stream(stream), t, nitems);
  else hipLaunchKernelGGL(sqdet::pack_many_kernel<float>, dim3(total_blocks), dim3(256), 0, as_stream(stream), t, nitems);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

extern "C" int sqdet_conv2d_nhwc_bwd_data(const void* dy, const void* w_packed_bwd, void* dx, int n, int h, int w, int cin,
                                          int cout, int k, int dtype, int dy_cstride, int dy_coffset, int accumulate,
                                          sqdet_stream_t stream) {
  // stride-1 SAME convs only (every trainable conv of the reference's nets on this path)
  SQDET_REQUIRE(k == 1 || k == 3, "conv2d_bwd_data: k must be 1 or 3 (stride 1, SAME)");
  return conv2d_launch_ex(dy, w_packed_bwd, nullptr, dx, n, h, w, cout, cin, k, 1, SQDET_PAD_SAME, 0, dtype, cin, 0,
                          dy_cstride, dy_coffset, accumulate, as_stream(stream));
}

extern "C" int sqdet_conv2d_nhwc_bwd_data_relu(const void* dy, const void* w_packed_bwd, void* dx, const void* relu_of, int n, int h,
                                               int w, int cin, int cout, int k, int dtype, int dy_cstride, int dy_coffset,
                                               int accumulate, sqdet_stream_t stream) {
  SQDET_REQUIRE(k == 1 || k == 3, "conv2d_bwd_data: k must be 1 or 3 (stride 1, SAME)");
  return conv2d_launch_masked(dy, w_packed_bwd, nullptr, dx, n, h, w, cout, cin, k, 1, SQDET_PAD_SAME, 0, dtype, cin, 0,
                              dy_cstride, dy_coffset, accumulate, relu_of, as_stream(stream));
}

extern "C" int sqdet_relu_bwd(const void* y, void* dy_inout, size_t count, int dtype, sqdet_stream_t stream) {
  SQDET_REQUIRE(dtype == SQDET_F16 || dtype == SQDET_F32, "relu_bwd: bad dtype");
  const size_t ev = 16 / dtype_size(dtype);
  SQDET_REQUIRE(y && dy_inout && count % ev == 0, "relu_bwd: bad arguments (count must be a multiple of 16 bytes)");
  const dim3 grid(grid_for(count / ev, 8192));
  if (dtype == SQDET_F16)
    hipLaunchKernelGGL(relu_bwd_kernel<f16>, grid, dim3(256), 0, as_stream(stream), (const f16*)y, (f16*)dy_inout, count / ev);
  else
    hipLaunchKernelGGL(relu_bwd_kernel<float>, grid, dim3(256), 0, as_stream(stream), (const float*)y, (float*)dy_inout, count / ev);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

extern "C" int sqdet_scale_mask(const void* x, const void* mask, void* y, float scale, size_t count, int dtype,
                                sqdet_stream_t stream) {
  SQDET_REQUIRE(dtype == SQDET_F16 || dtype == SQDET_F32, "scale_mask: bad dtype");
  const size_t ev = 16 / dtype_size(dtype);
  SQDET_REQUIRE(x && mask && y && count % ev == 0, "scale_mask: bad arguments (count must be a multiple of 16 bytes)");
  const dim3 grid(grid_for(count / ev, 8192));
  if (dtype == SQDET_F16)
    hipLaunchKernelGGL(scale_mask_kernel<f16>, grid, dim3(256), 0, as_stream(stream), (const f16*)x, (const f16*)mask, (f16*)y, scale, count / ev);
  else
    hipLaunchKernelGGL(scale_mask_kernel<float>, grid, dim3(256), 0, as_stream(stream), (const float*)x, (const float*)mask, (float*)y, scale, count / ev);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

extern "C" int sqdet_scale_mask_relu(const void* x, const void* mask, const void* relu_of, void* y, float scale, size_t count,
                                     int dtype, sqdet_stream_t stream) {
  SQDET_REQUIRE(dtype == SQDET_F16 || dtype == SQDET_F32, "scale_mask_relu: bad dtype");
  const size_t ev = 16 / dtype_size(dtype);
  SQDET_REQUIRE(x && mask && relu_of && y && count % ev == 0, "scale_mask_relu: bad arguments (count must be a multiple of 16 bytes)");
  const dim3 grid(grid_for(count / ev, 8192));
  if (dtype == SQDET_F16)
    hipLaunchKernelGGL(scale_mask_relu_kernel<f16>, grid, dim3(256), 0, as_stream(stream), (const f16*)x, (const f16*)mask,
                       (const f16*)relu_of, (f16*)y, scale, count / ev);
  else
    hipLaunchKernelGGL(scale_mask_relu_kernel<float>, grid, dim3(256), 0, as_stream(stream), (const float*)x, (const float*)mask,
                       (const float*)relu_of, (float*)y, scale, count / ev);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

extern "C" int sqdet_convert_scale(const void* src, int src_dtype, void* dst, int dst_dtype, float scale, size_t count,
                                   sqdet_stream_t stream) {
  SQDET_REQUIRE(src && dst && count % 4 == 0, "convert_scale: bad arguments (count must be a multiple of 4)");
  SQDET_REQUIRE((src_dtype == SQDET_F16 || src_dtype == SQDET_F32) && (dst_dtype == SQDET_F16 || dst_dtype == SQDET_F32),
                "convert_scale: bad dtype");
  const dim3 grid(grid_for(count / 4, 8192));
  hipStream_t st = as_stream(stream);
  if (src_dtype == SQDET_F16 && dst_dtype == SQDET_F32)
    hipLaunchKernelGGL((convert_scale_kernel<f16, float>), grid, dim3(256), 0, st, (const f16*)src, (float*)dst, scale, count / 4);
  else if (src_dtype == SQDET_F32 && dst_dtype == SQDET_F16)
    hipLaunchKernelGGL((convert_scale_kernel<float, f16>), grid, dim3(256), 0, st, (const float*)src, (f16*)dst, scale, count / 4);
  else if (src_dtype == SQDET_F32)
    hipLaunchKernelGGL((convert_scale_kernel<float, float>), grid, dim3(256), 0, st, (const float*)src, (float*)dst, scale, count / 4);
  else
    hipLaunchKernelGGL((convert_scale_kernel<f16, f16>), grid, dim3(256), 0, st, (const f16*)src, (f16*)dst, scale, count / 4);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

static int maxpool_bwd_launch(const void* x, const void* dy, void* dx, int n, int h, int w, int c, int k, int stride,
                              int pad_mode, int dtype, int relu, sqdet_stream_t stream);

extern "C" int sqdet_maxpool_nhwc_bwd(const void* x, const void* dy, void* dx, int n, int h, int w, int c, int k,
                                      int stride, int pad_mode, int dtype, sqdet_stream_t stream) {
  return maxpool_bwd_launch(x, dy, dx, n, h, w, c, k, stride, pad_mode, dtype, 0, stream);
}

extern "C" int sqdet_maxpool_nhwc_bwd_relu(const void* x, const void* dy, void* dx, int n, int h, int w, int c, int k,
                                           int stride, int pad_mode, int dtype, sqdet_stream_t stream) {
  return maxpool_bwd_launch(x, dy, dx, n, h, w, c, k, stride, pad_mode, dtype, 1, stream);
}

static int maxpool_bwd_launch(const void* x, const void* dy, void* dx, int n, int h, int w, int c, int k, int stride,
                              int pad_mode, int dtype, int relu, sqdet_stream_t stream) {
  SQDET_REQUIRE(dtype == SQDET_F16 || dtype == SQDET_F32, "maxpool_bwd: bad dtype");
  const int ev = 16 / (int)dtype_size(dtype);
  SQDET_REQUIRE(x && dy && dx && n > 0 && h > 0 && w > 0 && c > 0 && c % ev == 0 && k > 0 && stride > 0,
                "maxpool_bwd: bad arguments");
  const int Ho = out_size(h, k, stride, pad_mode), Wo = out_size(w, k, stride, pad_mode);
  const int pt = pad_before(h, k, stride, pad_mode), pl = pad_before(w, k, stride, pad_mode);
  if (k == 3 && stride == 2) {
    const int BA = (h + pt + 1) / 2, BB = (w + pl + 1) / 2;
    const dim3 grid2(grid_for((size_t)n * BA * BB * (c / ev), 16384));
    if (dtype == SQDET_F16)
      hipLaunchKernelGGL(maxpool3s2_bwd_kernel<f16>, grid2, dim3(256), 0, as_stream(stream), (const f16*)x, (const f16*)dy,
                         (f16*)dx, n, h, w, c, pt, pl, Ho, Wo, BA, BB, relu);
    else
      hipLaunchKernelGGL(maxpool3s2_bwd_kernel<float>, grid2, dim3(256), 0, as_stream(stream), (const float*)x,
                         (const float*)dy, (float*)dx, n, h, w, c, pt, pl, Ho, Wo, BA, BB, relu);
    SQDET_CHECK_HIP(hipGetLastError());
    return SQDET_OK;
  }
  const size_t total = (size_t)n * h * w * (c / ev);
  const dim3 grid(grid_for(total, 16384));
  if (dtype == SQDET_F16)
    hipLaunchKernelGGL(maxpool_bwd_kernel<f16>, grid, dim3(256), 0, as_stream(stream), (const f16*)x, (const f16*)dy, (f16*)dx,
                       n, h, w, c, k, stride, pt, pl, Ho, Wo, relu);
  else
    hipLaunchKernelGGL(maxpool_bwd_kernel<float>, grid, dim3(256), 0, as_stream(stream), (const float*)x, (const float*)dy,
                       (float*)dx, n, h, w, c, k, stride, pt, pl, Ho, Wo, relu);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

extern "C" int sqdet_maxpool_nhwc_bwd_idx(const unsigned char* window_index, const void* y, const void* dy, void* dx, int n, int h,
                                          int w, int c, int k, int stride, int pad_mode, int dtype, int relu,
                                          sqdet_stream_t stream) {
  SQDET_REQUIRE(dtype == SQDET_F16 || dtype == SQDET_F32, "maxpool_bwd_idx: bad dtype");
  const int ev = 16 / (int)dtype_size(dtype);
  SQDET_REQUIRE(window_index && dy && dx && (y || !relu) && n > 0 && h > 0 && w > 0 && c > 0 && c % ev == 0, "maxpool_bwd_idx: bad arguments");
  SQDET_UNSUPPORTED((k != 3 && k != 2) || stride != 2, "maxpool_bwd_idx: 3x3 and 2x2 windows of stride 2 only");
  SQDET_REQUIRE(k == 3 || pad_mode == SQDET_PAD_SAME || (pad_mode == SQDET_PAD_VALID && h >= 2 && w >= 2),
                "maxpool_bwd_idx: bad pad_mode, or VALID with h,w < 2");
  const int Ho = out_size(h, k, stride, pad_mode), Wo = out_size(w, k, stride, pad_mode);
  const int pt = pad_before(h, k, stride, pad_mode), pl = pad_before(w, k, stride, pad_mode);
  if (k == 2) {
    const int BA = (h + pt + 1) / 2, BB = (w + pl + 1) / 2;
    const dim3 grid(grid_for((size_t)n * BA * BB * (c / ev), 16384));
    if (dtype == SQDET_F16)
      hipLaunchKernelGGL(maxpool2s2_bwd_idx_kernel<f16>, grid, dim3(256), 0, as_stream(stream), window_index, (const f16*)y,
                         (const f16*)dy, (f16*)dx, n, h, w, c, pt, pl, Ho, Wo, BA, BB, relu);
    else
      hipLaunchKernelGGL(maxpool2s2_bwd_idx_kernel<float>, grid, dim3(256), 0, as_stream(stream), window_index, (const float*)y,
                         (const float*)dy, (float*)dx, n, h, w, c, pt, pl, Ho, Wo, BA, BB, relu);
    SQDET_CHECK_HIP(hipGetLastError());
    return SQDET_OK;
  }
  const int BA = (h + pt + 1) / 2, BB = (w + pl + 1) / 2;
  const dim3 grid(grid_for((size_t)n * BA * BB * (c / ev), 16384));
  if (dtype == SQDET_F16)
    hipLaunchKernelGGL(maxpool3s2_bwd_idx_kernel<f16>, grid, dim3(256), 0, as_stream(stream), window_index, (const f16*)y,
                       (const f16*)dy, (f16*)dx, n, h, w, c, pt, pl, Ho, Wo, BA, BB, relu);
  else
    hipLaunchKernelGGL(maxpool3s2_bwd_idx_kernel<float>, grid, dim3(256), 0, as_stream(stream), window_index, (const float*)y,
                       (const float*)dy, (float*)dx, n, h, w, c, pt, pl, Ho, Wo, BA, BB, relu);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

extern "C" int sqdet_sum_f32(const float* x, size_t count, float* out, sqdet_stream_t stream) {
  SQDET_REQUIRE(x && out && count > 0, "sum_f32: bad arguments");
  hipLaunchKernelGGL(sum_f32_kernel, dim3(1), dim3(1024), 0, as_stream(stream), x, count, out);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

extern "C" int sqdet_add_relu(const void* a, const void* b, void* y, size_t count, int dtype, sqdet_stream_t stream) {
  SQDET_REQUIRE(dtype == SQDET_F16 || dtype == SQDET_F32, "add_relu: bad dtype");
  const size_t ev = 16 / dtype_size(dtype);
  SQDET_REQUIRE(a && b && y && count % ev == 0, "add_relu: bad arguments (count must be a multiple of 16 bytes)");
  const dim3 grid(grid_for(count / ev, 8192));
  if (dtype == SQDET_F16)
    hipLaunchKernelGGL(add_relu_kernel<f16>, grid, dim3(256), 0, as_stream(stream), (const f16*)a, (const f16*)b, (f16*)y, count / ev);
  else
    hipLaunchKernelGGL(add_relu_kernel<float>, grid, dim3(256), 0, as_stream(stream), (const float*)a, (const float*)b, (float*)y, count / ev);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

extern "C" int sqdet_copy_channels(const void* x, void* y, size_t pixels, int c, int y_cstride, int y_coffset, int dtype,
                                   sqdet_stream_t stream) {
  SQDET_REQUIRE(dtype == SQDET_F16 || dtype == SQDET_F32, "copy_channels: bad dtype");
  const int ev = 16 / (int)dtype_size(dtype);
  SQDET_REQUIRE(x && y && pixels > 0 && c > 0 && c % ev == 0 && y_cstride % ev == 0 && y_coffset % ev == 0 && y_coffset >= 0 &&
                    y_coffset + c <= y_cstride, "copy_channels: channel counts / offsets must be multiples of 16 bytes");
  const dim3 grid(grid_for(pixels * (size_t)(c / ev), 8192));
  if (dtype == SQDET_F16)
    hipLaunchKernelGGL(copy_channels_kernel<f16>, grid, dim3(256), 0, as_stream(stream), (const f16*)x, (f16*)y, pixels, c / ev, y_cstride / ev, y_coffset / ev);
  else
    hipLaunchKernelGGL(copy_channels_kernel<float>, grid, dim3(256), 0, as_stream(stream), (const float*)x, (float*)y, pixels, c / ev, y_cstride / ev, y_coffset / ev);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

extern "C" int sqdet_dropout_mask(void* mask, size_t count, float keep_prob, uint64_t seed, int dtype, sqdet_stream_t stream) {
  SQDET_REQUIRE(dtype == SQDET_F16 || dtype == SQDET_F32, "dropout_mask: bad dtype");
  SQDET_REQUIRE(mask && count > 0 && keep_prob > 0.f && keep_prob <= 1.f, "dropout_mask: bad arguments");
  const dim3 grid(grid_for(count, 8192));
  if (dtype == SQDET_F16)
    hipLaunchKernelGGL(dropout_mask_kernel<f16>, grid, dim3(256), 0, as_stream(stream), (f16*)mask, count, keep_prob, (unsigned long long)seed);
  else
    hipLaunchKernelGGL(dropout_mask_kernel<float>, grid, dim3(256), 0, as_stream(stream), (float*)mask, count, keep_prob, (unsigned long long)seed);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

// Device -> PINNED HOST copy as a kernel (the destination is host memory mapped into the device's address space:
// hipHostMalloc / torch pin_memory).  hipMemcpyAsync device -> host was observed to hold the calling host thread until
// the stream reached the copy, which serialised the serving loop's two-stage pipeline; a kernel launch never does.
namespace sqdet {
__global__ void copy_to_mapped_host_kernel(const int4* __restrict__ src, int4* __restrict__ dst, size_t nv) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nv; i += (size_t)gridDim.x * blockDim.x) dst[i] = src[i];
}
}  // namespace sqdet

extern "C" int sqdet_copy_to_mapped_host(const void* src_device, void* dst_pinned_host, size_t nbytes, sqdet_stream_t stream) {
  SQDET_REQUIRE(src_device && dst_pinned_host && nbytes > 0 && nbytes % 16 == 0, "copy_to_mapped_host: bad arguments (16-byte multiples)");
  const size_t nv = nbytes / 16;
  size_t blocks = (nv + 255) / 256;
  if (blocks > 64) blocks = 64;
  hipLaunchKernelGGL(sqdet::copy_to_mapped_host_kernel, dim3((unsigned)blocks), dim3(256), 0, as_stream(stream),
                     (const int4*)src_device, (int4*)dst_pinned_host, nv);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}
