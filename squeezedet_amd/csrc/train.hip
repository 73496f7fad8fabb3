// Training-path kernels for gfx950 (float32 storage, the reference's training dtype):
//   conv backward-data   -- the forward conv kernel run on the 180-degree-rotated, in/out-swapped
//                           kernel (stride-1 SAME convs: every trainable conv of SqueezeDet);
//   conv backward-filter -- split-K GEMM over pixels on the exact-f32 MFMA, deterministic two-pass
//                           reduction (no atomics), + bias gradient;
//   ReLU / max-pool / dropout backward;
//   loss forward+backward (reference src/nn_skeleton.py:142-327: _add_interpretation_graph +
//                           _add_loss_graph) writing dL/dpreds;
//   Momentum update with per-variable clip_by_norm and weight decay (nn_skeleton.py:329-361).
// Compiled with -ffp-contract=off (the loss decode must match interpret_output op for op).
#include <math.h>

#include <vector>

#include "bn_fold.h"
#include "conv_common.h"
#include "item_table.h"

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

// (D)(v * scale), the product formed on its own.  Left to itself hipcc fuses a float32 multiply and the conversion to float16
// into v_fma_mixlo_f16(v, scale, +0), and (-0) + (+0) = +0: the sign of a zero product was lost -- on two of convert_scale's four
// lanes (the other two go through v_pk_mul_f32 + v_cvt_pk_f16_f32 and kept it) and in some of the loss kernel's stores.
template <typename D>
__device__ __forceinline__ D scaled_to(float v, float scale) {
  float p = v * scale;
  asm volatile("" : "+v"(p));
  return (D)p;
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

// ------------------------------------------------------------------ loss forward + backward
struct LossArgs {
  const void* preds;       // [B, cells, K*(C+5)], float32 or (mixed-precision form) float16
  const float* anchors;    // [A,4] float32
  const float* mask;       // [B,A]
  const float* delta_in;   // [B,A,4]
  const float* box_in;     // [B,A,4] (cx,cy,w,h)
  const float* labels;     // [B,A,C]
  float* dpreds;           // [B, cells, K*(C+5)]
  f16* g16;                // mixed-precision form: (float16)(dpreds * gscale), the gradient the float16 backward starts from
  float gscale;            // (the loss scale)
  float* losses3;
  float* ious;             // [B,A]
  float* partial;          // [blocks][4]: class, conf, bbox loss partial sums (+ unused)
  int B, cells, K, C;
  int Bmean;               // divisor of the confidence loss's reduce_mean over the batch (nn_skeleton.py:304-312): B, or the
                           // GLOBAL batch when N replicas of batch B compute one graph of batch N*B (SURVEY.md 8e option b)
  float w1, h1, thr, slope, eps;
  float coef_class, coef_pos, coef_neg, coef_bbox;
  float num_obj;           // sum(mask) over the whole batch (host computed from the label tensors) ...
  const float* num_obj_dev;   // ... or, when not NULL, read from the device (sqdet_sum_f32 of the mask: no host round trip)
};

template <typename PT>
__global__ __launch_bounds__(256) void loss_kernel(LossArgs a) {
  const float nobj = a.num_obj_dev ? a.num_obj_dev[0] : a.num_obj;
  __shared__ float red[3][256];
  const int A = a.cells * a.K;
  const int ch = a.K * (a.C + 5);
  const long total = (long)a.B * A;
  float l_class = 0.f, l_conf = 0.f, l_bbox = 0.f;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int b = (int)(idx / A);
    const int an = (int)(idx - (long)b * A);
    const int cell = an / a.K, k = an - cell * a.K;
    const PT* p = reinterpret_cast<const PT*>(a.preds) + ((size_t)b * a.cells + cell) * ch;
    float* dp = a.dpreds + ((size_t)b * a.cells + cell) * ch;
    f16* gp = a.g16 ? a.g16 + ((size_t)b * a.cells + cell) * ch : nullptr;
    // float32 dpreds, and -- mixed precision -- its loss-scaled float16 copy (convert_scale_kernel's expression) in the same pass
    auto put = [&](int off, float v) {
      dp[off] = v;
      if (sizeof(PT) == 2) gp[off] = scaled_to<f16>(v, a.gscale);
    };
    const float m = a.mask[idx];
    // class probabilities (softmax) and their loss (nn_skeleton.py:150-160, 292-299)
    const PT* lg = p + k * a.C;
    float mx = (float)lg[0];
    for (int c = 1; c < a.C; ++c) mx = fmaxf(mx, (float)lg[c]);
    float sum = expf((float)lg[0] - mx);
    for (int c = 1; c < a.C; ++c) sum = sum + expf((float)lg[c] - mx);
    const float inv = 1.0f / sum;
    float gdotp = 0.f;
    for (int c = 0; c < a.C; ++c) {
      const float pc = expf((float)lg[c] - mx) * inv;
      const float lab = a.labels[idx * a.C + c];
      l_class += (lab * (-logf(pc + a.eps)) + (1.0f - lab) * (-logf(1.0f - pc + a.eps))) * m * a.coef_class;
      const float gc = m * a.coef_class / nobj * (-lab / (pc + a.eps) + (1.0f - lab) / (1.0f - pc + a.eps));
      gdotp += gc * pc;
    }
    for (int c = 0; c < a.C; ++c) {
      const float pc = expf((float)lg[c] - mx) * inv;
      const float lab = a.labels[idx * a.C + c];
      const float gc = m * a.coef_class / nobj * (-lab / (pc + a.eps) + (1.0f - lab) / (1.0f - pc + a.eps));
      put(k * a.C + c, pc * (gc - gdotp));
    }
    // decode (as interpret_output) -> IoU with the ground-truth box (nn_skeleton.py:240-269)
    const float zc = (float)p[a.K * a.C + k];
    const float conf = 1.0f / (1.0f + expf(-zc));
    const PT* dlp = p + a.K * (a.C + 1) + 4 * k;
    const float dl[4] = {(float)dlp[0], (float)dlp[1], (float)dlp[2], (float)dlp[3]};
    const f32x4 anc = *reinterpret_cast<const f32x4*>(a.anchors + (size_t)an * 4);
    const float cx = anc[0] + dl[0] * anc[2];
    const float cy = anc[1] + dl[1] * anc[3];
    const float ew = dl[2] > a.thr ? a.slope * ((dl[2] - a.thr) + 1.0f) : expf(dl[2]);
    const float eh = dl[3] > a.thr ? a.slope * ((dl[3] - a.thr) + 1.0f) : expf(dl[3]);
    const float bw = anc[2] * ew, bh = anc[3] * eh;
    float xmin = fminf(fmaxf(0.0f, cx - bw / 2.0f), a.w1), ymin = fminf(fmaxf(0.0f, cy - bh / 2.0f), a.h1);
    float xmax = fmaxf(fminf(a.w1, cx + bw / 2.0f), 0.0f), ymax = fmaxf(fminf(a.h1, cy + bh / 2.0f), 0.0f);
    const float w2 = xmax - xmin + 1.0f, h2 = ymax - ymin + 1.0f;
    const float dcx = xmin + 0.5f * w2, dcy = ymin + 0.5f * h2;
    // bbox_transform of det box and of the GT box (utils/util.py:167-179), _tensor_iou (:241-262)
    const float ax0 = dcx - w2 / 2.0f, ay0 = dcy - h2 / 2.0f, ax1 = dcx + w2 / 2.0f, ay1 = dcy + h2 / 2.0f;
    const f32x4 gb = *reinterpret_cast<const f32x4*>(a.box_in + idx * 4);
    const float bx0 = gb[0] - gb[2] / 2.0f, by0 = gb[1] - gb[3] / 2.0f, bx1 = gb[0] + gb[2] / 2.0f, by1 = gb[1] + gb[3] / 2.0f;
    const float iw = fmaxf(0.0f, fminf(ax1, bx1) - fmaxf(ax0, bx0));
    const float ih = fmaxf(0.0f, fminf(ay1, by1) - fmaxf(ay0, by0));
    const float inter = iw * ih;
    const float uni = (ax1 - ax0) * (ay1 - ay0) + (bx1 - bx0) * (by1 - by0) - inter;
    const float iou = inter / (uni + a.eps) * m;
    a.ious[idx] = iou;
    // confidence loss (:304-312): mean over the batch of sum_a (iou-conf)^2 * w_a
    const float wgt = m * a.coef_pos / nobj + (1.0f - m) * a.coef_neg / ((float)A - nobj);
    const float dc = iou - conf;
    l_conf += dc * dc * wgt / (float)a.Bmean;
    put(a.K * a.C + k, 2.0f * (conf - iou) * wgt / (float)a.Bmean * conf * (1.0f - conf));
    // bbox loss (:317-323)
    for (int d = 0; d < 4; ++d) {
      const float df = m * (dl[d] - a.delta_in[idx * 4 + d]);
      l_bbox += a.coef_bbox * df * df / nobj;
      put(a.K * (a.C + 1) + 4 * k + d, 2.0f * a.coef_bbox * m * df / nobj);
    }
  }
  l_class = l_class / nobj;
  red[0][threadIdx.x] = l_class; red[1][threadIdx.x] = l_conf; red[2][threadIdx.x] = l_bbox;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) {
      red[0][threadIdx.x] += red[0][threadIdx.x + off];
      red[1][threadIdx.x] += red[1][threadIdx.x + off];
      red[2][threadIdx.x] += red[2][threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x < 4) a.partial[blockIdx.x * 4 + threadIdx.x] = threadIdx.x < 3 ? red[threadIdx.x][0] : 0.f;
}

// losses3[j] = sum over the loss kernel's workgroups of partial[b][j]: wave j of one workgroup, lane l takes b = l, l + 64, ..
// in ascending order, then a fixed xor tree -- deterministic.  (One thread per output walking up to 512 dependent loads took
// 40 us, and a device-to-device copy of the three floats followed it.)
__global__ __launch_bounds__(256) void loss_finish_kernel(const float* __restrict__ partial, float* __restrict__ losses3, int blocks) {
  const int j = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float s = 0.f;
  for (int b = lane; b < blocks; b += 64) s += partial[b * 4 + j];
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0 && j < 3) losses3[j] = s;
}

// ------------------------------------------------------------------ distillation (OURS: not in the reference)
// A teacher's preds as a second target (sqdet_distill_fwd_bwd; the definition stands in include/sqdet.h and, sequentially, in
// tests/distill_reference.py).  loss_kernel's shape: a thread per anchor in a grid-stride loop, per-thread sums in index order,
// the LDS tree, at most 512 partials, loss_finish_kernel.  Runs after the loss launch: every channel's own gradient g is formed
// completely, then dpreds = dpreds + g and -- float16 student -- the loss-scaled float16 copy of that sum.  The softmaxes are
// re-evaluated per class instead of kept in a per-thread array (C is a run-time value: an array would live in scratch).
// Every division by the batch is the last operation of its expression and the sums are divided once per thread, so that
// global_batch = 2 * batch halves every output exactly.
struct DistillArgs {
  const void* preds;       // student [B, cells, K*(C+5)], float32 or float16
  const void* teacher;     // teacher, the same shape, float32 or float16
  float* dpreds;           // [B, cells, K*(C+5)], read and written
  f16* g16;                // float16 student: (float16)(dpreds * gscale)
  float gscale;
  float* partial;          // [blocks][4]: class, conf, box partial sums (+ unused)
  int B, cells, K, C;
  float Bg, BgA;           // (float)global batch, and times the anchors per image
  float T, c_cls, c_conf, c_box, floor;
};

__device__ __forceinline__ float softplusf(float z) { return fmaxf(z, 0.0f) + log1pf(expf(-fabsf(z))); }

template <typename PT, typename TT>
__global__ __launch_bounds__(256) void distill_kernel(DistillArgs a) {
  __shared__ float red[3][256];
  const int A = a.cells * a.K;
  const int ch = a.K * (a.C + 5);
  const long total = (long)a.B * A;
  float l_cls = 0.f, l_conf = 0.f, l_box = 0.f;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int b = (int)(idx / A);
    const int an = (int)(idx - (long)b * A);
    const int cell = an / a.K, k = an - cell * a.K;
    const size_t base = ((size_t)b * a.cells + cell) * ch;
    const PT* s = reinterpret_cast<const PT*>(a.preds) + base;
    const TT* t = reinterpret_cast<const TT*>(a.teacher) + base;
    float* dp = a.dpreds + base;
    f16* gp = a.g16 ? a.g16 + base : nullptr;
    auto add = [&](int off, float g) {
      const float v = dp[off] + g;
      dp[off] = v;
      if (sizeof(PT) == 2) gp[off] = scaled_to<f16>(v, a.gscale);
    };
    // teacher confidence -> the anchor's weight; the confidence term
    const float us = (float)s[a.K * a.C + k], ut = (float)t[a.K * a.C + k];
    const float cs = 1.0f / (1.0f + expf(-us)), ct = 1.0f / (1.0f + expf(-ut));
    const float w = ct >= a.floor ? ct : 0.0f;
    l_conf += ct * (ut - us) + softplusf(us) - softplusf(ut);
    add(a.K * a.C + k, a.c_conf * (cs - ct) / a.BgA);
    // class term: KL(q || p) of the tempered softmaxes, through max-subtracted log-softmax
    const PT* zs = s + k * a.C;
    const TT* zt = t + k * a.C;
    float ms = (float)zs[0] / a.T, mt = (float)zt[0] / a.T;
    for (int c = 1; c < a.C; ++c) { ms = fmaxf(ms, (float)zs[c] / a.T); mt = fmaxf(mt, (float)zt[c] / a.T); }
    float ss = expf((float)zs[0] / a.T - ms), st = expf((float)zt[0] / a.T - mt);
    for (int c = 1; c < a.C; ++c) { ss = ss + expf((float)zs[c] / a.T - ms); st = st + expf((float)zt[c] / a.T - mt); }
    const float ls = logf(ss), lt = logf(st);
    float kl = 0.f;
    for (int c = 0; c < a.C; ++c) {
      const float lp = ((float)zs[c] / a.T - ms) - ls, lq = ((float)zt[c] / a.T - mt) - lt;
      const float p = expf(lp), q = expf(lq);
      kl += q * (lq - lp);
      add(k * a.C + c, a.c_cls * a.T * w * (p - q) / a.Bg);
    }
    l_cls += w * kl;
    // box term: squared error on the four deltas
    const PT* ds = s + a.K * (a.C + 1) + 4 * k;
    const TT* dt = t + a.K * (a.C + 1) + 4 * k;
    float sq = 0.f;
    for (int d = 0; d < 4; ++d) {
      const float df = (float)ds[d] - (float)dt[d];
      sq += df * df;
      add(a.K * (a.C + 1) + 4 * k + d, 2.0f * a.c_box * w * df / a.Bg);
    }
    l_box += w * sq;
  }
  red[0][threadIdx.x] = a.c_cls * a.T * a.T * l_cls / a.Bg;
  red[1][threadIdx.x] = a.c_conf * l_conf / a.BgA;
  red[2][threadIdx.x] = a.c_box * l_box / a.Bg;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) {
      red[0][threadIdx.x] += red[0][threadIdx.x + off];
      red[1][threadIdx.x] += red[1][threadIdx.x + off];
      red[2][threadIdx.x] += red[2][threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x < 4) a.partial[blockIdx.x * 4 + threadIdx.x] = threadIdx.x < 3 ? red[threadIdx.x][0] : 0.f;
}

// ------------------------------------------------------------------ loss with options (OURS: not in the reference)
// loss_kernel with two of its three terms replaceable (sqdet_loss_fwd_bwd_opt); the confidence term, the
// decode, `ious`, the partial sums and loss_finish_kernel are loss_kernel's, expression for expression.
//
// Box term, box_loss 1..4: coef_bbox * sum_a m * (1 - X) / num_objects on the corners loss_kernel already has -- the
// prediction (ax0, ay0, ax1, ay1) = the clipped decoded box with its '+1' sides, the ground truth (bx0 .. by1) -- so that the
// term's IoU is the float32 value stored in `ious`.  With pw, ph / gw, gh the sides, Cw, Ch the sides of the enclosing box,
// rho2 the squared distance of the centres:
//   iou   X = IoU = inter / (uni + eps)
//   giou  X = IoU - (Cw*Ch - uni) / (Cw*Ch + eps)
//   diou  X = IoU - rho2 / (Cw^2 + Ch^2 + eps)
//   ciou  X = IoU - rho2 / (Cw^2 + Ch^2 + eps) - alpha * v,  v = 4/pi^2 * (atan(gw/gh) - atan(pw/ph))^2,
//         alpha = v / (1 - IoU + v + eps), a constant in the backward pass; dv/dpw = -8/pi^2 * (..) * ph / (pw^2 + ph^2) (the true one).
// An anchor with m == 0 takes no part in it (its ground truth is all zeros) and gets zero delta gradients.
//
// Backward: dX / d(corner) by the quotient rule on the expressions above, then the chain through  ax0 = xmin, ax1 = xmax + 1,
// xmin / xmax = clip(cx -+ bw/2, 0, w1), bw = anc_w * safe_exp(d2) (derivative exp(d2), or `slope` on the linear branch d2 > thr),
// cx = anc_x + d0 * anc_w:   dL/dd0 = anc_w * (g_x0 + g_x1),  dL/dd2 = anc_w * safe_exp'(d2) / 2 * (g_x1 - g_x0); y alike.
//
// TIE RULE (one rule for every min, max and clip): a coordinate of the prediction receives gradient through a min / max / clip
// only where it is STRICTLY the selected argument; at equality the other argument -- the ground truth's coordinate, the 0 of
// the intersection's max(0, .), the image border -- takes it, and nothing flows.  So
//   min(ax1, bx1) passes to ax1 iff ax1 < bx1, max(ax0, bx0) to ax0 iff ax0 > bx0 (intersection; and only if its side is > 0),
//   max(ax1, bx1) passes to ax1 iff ax1 > bx1, min(ax0, bx0) to ax0 iff ax0 < bx0 (enclosing box),
//   an edge passes the clip iff 0 < cx -+ bw/2 < w1: an edge exactly on the border counts as clipped.
// tests/loss_options_reference.py restates the same rule in NumPy.
//
// Class term, focal_gamma g > 0:  lab * (1-pc)^g * (-log(pc+eps)) + (1-lab) * pc^g * (-log(1-pc+eps)), its derivative in pc
// exact, the modulating factor's included: d(b^g)/db = g * b^g / b, taken as 0 where b == 0 (there the other factor, the
// log, is 0 as well).  g == 0 is the reference expression itself, no powf.
struct LossOpt { int box_loss; float gamma; };

// one class's term f(pc) and df/dpc
__device__ __forceinline__ void focal_term(float pc, float lab, float eps, float g, float& f, float& df) {
  const float lp = -logf(pc + eps), lq = -logf(1.0f - pc + eps);
  if (g == 0.f) {
    f = lab * lp + (1.0f - lab) * lq;
    df = -lab / (pc + eps) + (1.0f - lab) / (1.0f - pc + eps);
    return;
  }
  const float q = fmaxf(1.0f - pc, 0.0f);
  const float qg = powf(q, g), pg = powf(pc, g);
  const float dqg = q > 0.f ? g * qg / q : 0.f, dpg = pc > 0.f ? g * pg / pc : 0.f;
  f = lab * (qg * lp) + (1.0f - lab) * (pg * lq);
  df = lab * (-dqg * lp - qg / (pc + eps)) + (1.0f - lab) * (dpg * lq + pg / (1.0f - pc + eps));
}

template <typename PT>
__global__ __launch_bounds__(256) void loss_opt_kernel(LossArgs a, LossOpt o) {
  const float nobj = a.num_obj_dev ? a.num_obj_dev[0] : a.num_obj;
  __shared__ float red[3][256];
  const int A = a.cells * a.K;
  const int ch = a.K * (a.C + 5);
  const long total = (long)a.B * A;
  float l_class = 0.f, l_conf = 0.f, l_bbox = 0.f;
  for (long idx = (long)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (long)gridDim.x * blockDim.x) {
    const int b = (int)(idx / A);
    const int an = (int)(idx - (long)b * A);
    const int cell = an / a.K, k = an - cell * a.K;
    const PT* p = reinterpret_cast<const PT*>(a.preds) + ((size_t)b * a.cells + cell) * ch;
    float* dp = a.dpreds + ((size_t)b * a.cells + cell) * ch;
    f16* gp = a.g16 ? a.g16 + ((size_t)b * a.cells + cell) * ch : nullptr;
    auto put = [&](int off, float v) {
      dp[off] = v;
      if (sizeof(PT) == 2) gp[off] = scaled_to<f16>(v, a.gscale);
    };
    const float m = a.mask[idx];
    // class probabilities (softmax) and the class term
    const PT* lg = p + k * a.C;
    float mx = (float)lg[0];
    for (int c = 1; c < a.C; ++c) mx = fmaxf(mx, (float)lg[c]);
    float sum = expf((float)lg[0] - mx);
    for (int c = 1; c < a.C; ++c) sum = sum + expf((float)lg[c] - mx);
    const float inv = 1.0f / sum;
    float gdotp = 0.f;
    if (o.gamma != 0.f && m == 0.f) {
      // an unlabelled anchor's term and gradient are m * (finite) = 0: no powf for it (nearly every anchor: the focal launch
      // took 46 us against 25 us before this branch, batch 20)
      for (int c = 0; c < a.C; ++c) put(k * a.C + c, 0.f);
    } else {
      for (int c = 0; c < a.C; ++c) {
        const float pc = expf((float)lg[c] - mx) * inv;
        float f, df;
        focal_term(pc, a.labels[idx * a.C + c], a.eps, o.gamma, f, df);
        l_class += f * m * a.coef_class;
        const float gc = m * a.coef_class / nobj * df;
        gdotp += gc * pc;
      }
      for (int c = 0; c < a.C; ++c) {
        const float pc = expf((float)lg[c] - mx) * inv;
        float f, df;
        focal_term(pc, a.labels[idx * a.C + c], a.eps, o.gamma, f, df);
        const float gc = m * a.coef_class / nobj * df;
        put(k * a.C + c, pc * (gc - gdotp));
      }
    }
    // decode -> IoU with the ground-truth box: loss_kernel's expressions
    const float zc = (float)p[a.K * a.C + k];
    const float conf = 1.0f / (1.0f + expf(-zc));
    const PT* dlp = p + a.K * (a.C + 1) + 4 * k;
    const float dl[4] = {(float)dlp[0], (float)dlp[1], (float)dlp[2], (float)dlp[3]};
    const f32x4 anc = *reinterpret_cast<const f32x4*>(a.anchors + (size_t)an * 4);
    const float cx = anc[0] + dl[0] * anc[2];
    const float cy = anc[1] + dl[1] * anc[3];
    const float ew = dl[2] > a.thr ? a.slope * ((dl[2] - a.thr) + 1.0f) : expf(dl[2]);
    const float eh = dl[3] > a.thr ? a.slope * ((dl[3] - a.thr) + 1.0f) : expf(dl[3]);
    const float bw = anc[2] * ew, bh = anc[3] * eh;
    const float rx0 = cx - bw / 2.0f, ry0 = cy - bh / 2.0f, rx1 = cx + bw / 2.0f, ry1 = cy + bh / 2.0f;
    float xmin = fminf(fmaxf(0.0f, rx0), a.w1), ymin = fminf(fmaxf(0.0f, ry0), a.h1);
    float xmax = fmaxf(fminf(a.w1, rx1), 0.0f), ymax = fmaxf(fminf(a.h1, ry1), 0.0f);
    const float w2 = xmax - xmin + 1.0f, h2 = ymax - ymin + 1.0f;
    const float dcx = xmin + 0.5f * w2, dcy = ymin + 0.5f * h2;
    const float ax0 = dcx - w2 / 2.0f, ay0 = dcy - h2 / 2.0f, ax1 = dcx + w2 / 2.0f, ay1 = dcy + h2 / 2.0f;
    const f32x4 gb = *reinterpret_cast<const f32x4*>(a.box_in + idx * 4);
    const float bx0 = gb[0] - gb[2] / 2.0f, by0 = gb[1] - gb[3] / 2.0f, bx1 = gb[0] + gb[2] / 2.0f, by1 = gb[1] + gb[3] / 2.0f;
    const float iwr = fminf(ax1, bx1) - fmaxf(ax0, bx0), ihr = fminf(ay1, by1) - fmaxf(ay0, by0);
    const float iw = fmaxf(0.0f, iwr);
    const float ih = fmaxf(0.0f, ihr);
    const float inter = iw * ih;
    const float uni = (ax1 - ax0) * (ay1 - ay0) + (bx1 - bx0) * (by1 - by0) - inter;
    const float iou1 = inter / (uni + a.eps);
    const float iou = iou1 * m;
    a.ious[idx] = iou;
    // confidence loss: loss_kernel's
    const float wgt = m * a.coef_pos / nobj + (1.0f - m) * a.coef_neg / ((float)A - nobj);
    const float dc = iou - conf;
    l_conf += dc * dc * wgt / (float)a.Bmean;
    put(a.K * a.C + k, 2.0f * (conf - iou) * wgt / (float)a.Bmean * conf * (1.0f - conf));
    // box term
    const int doff = a.K * (a.C + 1) + 4 * k;
    if (o.box_loss == 0) {
      for (int d = 0; d < 4; ++d) {
        const float df = m * (dl[d] - a.delta_in[idx * 4 + d]);
        l_bbox += a.coef_bbox * (df * df);          // (divided by num_objects once, below, as the class term is)
        put(doff + d, 2.0f * a.coef_bbox * m * df / nobj);
      }
    } else if (m == 0.f) {
      for (int d = 0; d < 4; ++d) put(doff + d, 0.f);
    } else {
      // corner order x0, y0, x1, y1; every flag is the tie rule of the header comment
      const float pw = ax1 - ax0, ph = ay1 - ay0, gw = bx1 - bx0, gh = by1 - by0;
      const float fx = iwr > 0.f ? 1.f : 0.f, fy = ihr > 0.f ? 1.f : 0.f;
      const float di[4] = {ax0 > bx0 ? -fx * ih : 0.f, ay0 > by0 ? -fy * iw : 0.f, ax1 < bx1 ? fx * ih : 0.f, ay1 < by1 ? fy * iw : 0.f};
      const float da[4] = {-ph, -pw, ph, pw};
      const float ue = uni + a.eps;
      float X = iou1, du[4], dX[4];
      for (int j = 0; j < 4; ++j) {
        du[j] = da[j] - di[j];
        dX[j] = (di[j] - iou1 * du[j]) / ue;
      }
      if (o.box_loss >= 2) {
        const float Cw = fmaxf(ax1, bx1) - fminf(ax0, bx0), Ch = fmaxf(ay1, by1) - fminf(ay0, by0);
        const float sx0 = ax0 < bx0 ? -1.f : 0.f, sy0 = ay0 < by0 ? -1.f : 0.f, sx1 = ax1 > bx1 ? 1.f : 0.f, sy1 = ay1 > by1 ? 1.f : 0.f;
        if (o.box_loss == 2) {
          const float Ca = Cw * Ch, ce = Ca + a.eps;
          const float T = (Ca - uni) / ce;
          const float dC[4] = {sx0 * Ch, sy0 * Cw, sx1 * Ch, sy1 * Cw};
          X = X - T;
          for (int j = 0; j < 4; ++j) dX[j] = dX[j] - ((dC[j] - du[j]) - T * dC[j]) / ce;
        } else {
          const float c2e = (Cw * Cw + Ch * Ch) + a.eps;
          const float ex = (ax0 + ax1) * 0.5f - (bx0 + bx1) * 0.5f, ey = (ay0 + ay1) * 0.5f - (by0 + by1) * 0.5f;
          const float D = (ex * ex + ey * ey) / c2e;
          const float dr[4] = {ex, ey, ex, ey};
          const float dc2[4] = {2.0f * Cw * sx0, 2.0f * Ch * sy0, 2.0f * Cw * sx1, 2.0f * Ch * sy1};
          X = X - D;
          for (int j = 0; j < 4; ++j) dX[j] = dX[j] - (dr[j] - D * dc2[j]) / c2e;
          if (o.box_loss == 4) {
            const float k4 = 0.40528473456935109f;       // 4 / pi^2
            const float dat = atanf(gw / gh) - atanf(pw / ph);
            const float v = k4 * dat * dat;
            const float alpha = v / (((1.0f - iou1) + v) + a.eps);
            const float s2 = pw * pw + ph * ph;
            const float vw = -2.0f * k4 * dat * ph / s2, vh = 2.0f * k4 * dat * pw / s2;      // dv/dpw, dv/dph
            const float dv[4] = {-vw, -vh, vw, vh};
            X = X - alpha * v;
            for (int j = 0; j < 4; ++j) dX[j] = dX[j] - alpha * dv[j];
          }
        }
      }
      const float sc = a.coef_bbox * m / nobj;
      l_bbox += a.coef_bbox * m * (1.0f - X);
      const float gx0 = rx0 > 0.f && rx0 < a.w1 ? -sc * dX[0] : 0.f, gy0 = ry0 > 0.f && ry0 < a.h1 ? -sc * dX[1] : 0.f;
      const float gx1 = rx1 > 0.f && rx1 < a.w1 ? -sc * dX[2] : 0.f, gy1 = ry1 > 0.f && ry1 < a.h1 ? -sc * dX[3] : 0.f;
      const float dew = dl[2] > a.thr ? a.slope : ew, deh = dl[3] > a.thr ? a.slope : eh;
      put(doff + 0, anc[2] * (gx0 + gx1));
      put(doff + 1, anc[3] * (gy0 + gy1));
      put(doff + 2, 0.5f * anc[2] * dew * (gx1 - gx0));
      put(doff + 3, 0.5f * anc[3] * deh * (gy1 - gy0));
    }
  }
  l_class = l_class / nobj;
  l_bbox = l_bbox / nobj;
  red[0][threadIdx.x] = l_class; red[1][threadIdx.x] = l_conf; red[2][threadIdx.x] = l_bbox;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) {
      red[0][threadIdx.x] += red[0][threadIdx.x + off];
      red[1][threadIdx.x] += red[1][threadIdx.x + off];
      red[2][threadIdx.x] += red[2][threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x < 4) a.partial[blockIdx.x * 4 + threadIdx.x] = threadIdx.x < 3 ? red[threadIdx.x][0] : 0.f;
}

// ------------------------------------------------------------------ optimizer
// Segment table: variable v occupies [seg[v].off, +count) of the flat parameter / gradient / momentum
// buffers.  Pass 1 adds the weight-decay gradient and writes per-block partial sums of squares; pass 2
// (one block) finishes the norms in a fixed order; pass 3 clips per variable and applies Momentum.
struct OptSeg { long off; long count; float decay; int first_block; int nblocks; };

__global__ __launch_bounds__(256) void opt_sumsq_kernel(const OptSeg* __restrict__ segs, const int* __restrict__ block_seg,
                                                        const float* __restrict__ w, float* __restrict__ g,
                                                        double* __restrict__ partial, float grad_scale) {
  __shared__ double red[256];
  const int v = block_seg[blockIdx.x];
  const OptSeg s = segs[v];
  const int lb = blockIdx.x - s.first_block;
  double acc = 0.0;
  for (long i = (long)lb * 256 + threadIdx.x; i < s.count; i += (long)s.nblocks * 256) {
    float gi = g[s.off + i] * grad_scale;   // grad_scale = 1/world_size after a SUM all-reduce
    if (s.decay != 0.f) gi = gi + s.decay * w[s.off + i];
    g[s.off + i] = gi;
    acc += (double)gi * (double)gi;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// one block: per-variable clip factors + the overflow flag of mixed-precision training (a non-finite gradient norm in
// ANY variable: flag[0] = 1 and the apply kernel leaves every parameter and momentum untouched)
__global__ void opt_norm_kernel(const OptSeg* __restrict__ segs, const double* __restrict__ partial, float* __restrict__ scale,
                                int nvars, float max_norm, int* __restrict__ flag, int* __restrict__ found_inf) {
  int bad = 0;
  for (int v = threadIdx.x; v < nvars; v += blockDim.x) {
    double s = 0.0;
    for (int b = 0; b < segs[v].nblocks; ++b) s += partial[segs[v].first_block + b];
    const float nrm = (float)sqrt(s);
    if (!(nrm <= 3.0e38f)) bad = 1;               // inf or NaN
    scale[v] = max_norm / fmaxf(nrm, max_norm);   // tf.clip_by_norm: g * clip / max(||g||, clip)
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    flag[0] = bad;
    if (found_inf) found_inf[0] = bad;
  }
}

__global__ __launch_bounds__(256) void opt_apply_kernel(const OptSeg* __restrict__ segs, const int* __restrict__ block_seg,
                                                        float* __restrict__ w, const float* __restrict__ g,
                                                        float* __restrict__ accum, const float* __restrict__ scale,
                                                        float lr, float momentum, const int* __restrict__ flag) {
  if (flag[0]) return;   // overflowed step: skipped
  const int v = block_seg[blockIdx.x];
  const OptSeg s = segs[v];
  const int lb = blockIdx.x - s.first_block;
  const float sc = scale[v];
  for (long i = (long)lb * 256 + threadIdx.x; i < s.count; i += (long)s.nblocks * 256) {
    const float gc = g[s.off + i] * sc;
    const float ac = momentum * accum[s.off + i] + gc;   // MomentumOptimizer: accum = m*accum + g ; var -= lr*accum
    accum[s.off + i] = ac;
    w[s.off + i] = w[s.off + i] - lr * ac;
  }
}

// ---- the optimizer with options (sqdet_optimizer_step_opt): the same three passes over the same block table.
// Pass 1 is opt_sumsq_kernel with the coupled decay switched off under AdamW (same partition, same order: COUPLE gives its bits).
template <bool COUPLE>
__global__ __launch_bounds__(256) void opt_sumsq_opt_kernel(const OptSeg* __restrict__ segs, const int* __restrict__ block_seg,
                                                            const float* __restrict__ w, float* __restrict__ g,
                                                            double* __restrict__ partial, float grad_scale) {
  __shared__ double red[256];
  const int v = block_seg[blockIdx.x];
  const OptSeg s = segs[v];
  const int lb = blockIdx.x - s.first_block;
  double acc = 0.0;
  for (long i = (long)lb * 256 + threadIdx.x; i < s.count; i += (long)s.nblocks * 256) {
    float gi = g[s.off + i] * grad_scale;
    if (COUPLE && s.decay != 0.f) gi = gi + s.decay * w[s.off + i];
    g[s.off + i] = gi;
    acc += (double)gi * (double)gi;
  }
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}

// Pass 2 (one block of 256): the clip factors, the overflow flag and -- on a step that applies -- the device state
// state[0..3) = (t, beta1^t, beta2^t) advanced by one update and the three float32 scalars pass 3 reads,
// derived[0..3) = (1 / (1 - beta1^t), 1 / (1 - beta2^t), 1 - d), each formed in float64 and rounded once (the first two under AdamW,
// the third with an EMA: nothing else reads them).  Global clip: the
// per-variable float64 sums are added in variable-index order (laps of 256 through LDS, one thread adding).
__global__ __launch_bounds__(256) void opt_norm_opt_kernel(const OptSeg* __restrict__ segs, const double* __restrict__ partial,
                                                           float* __restrict__ scale, int nvars, float max_norm, int global_clip,
                                                           int adamw, double beta1, double beta2, double ema_decay, int ema_warmup,
                                                           double* __restrict__ state, float* __restrict__ derived,
                                                           int* __restrict__ flag, int* __restrict__ found_inf) {
  __shared__ double vsum[256];
  __shared__ float gfactor;
  int bad = 0;
  double S = 0.0;                                   // (thread 0)
  for (int base = 0; base < nvars; base += 256) {   // uniform trip count: the barriers below are reached by every thread
    const int v = base + threadIdx.x;
    if (v < nvars) {
      double s = 0.0;
      for (int b = 0; b < segs[v].nblocks; ++b) s += partial[segs[v].first_block + b];
      const float nrm = (float)sqrt(s);
      if (!(nrm <= 3.0e38f)) bad = 1;               // inf or NaN
      if (!global_clip) scale[v] = max_norm / fmaxf(nrm, max_norm);
      vsum[threadIdx.x] = s;
    }
    if (global_clip) {
      __syncthreads();
      if (threadIdx.x == 0) {
        const int n = nvars - base < 256 ? nvars - base : 256;
        for (int k = 0; k < n; ++k) S += vsum[k];
      }
      __syncthreads();
    }
  }
  if (global_clip) {
    if (threadIdx.x == 0) {
      const float N = (float)sqrt(S);               // tf.clip_by_global_norm: every g * clip / max(||all g||, clip)
      if (!(N <= 3.0e38f)) bad = 1;
      gfactor = max_norm / fmaxf(N, max_norm);
    }
    __syncthreads();
    const float f = gfactor;
    for (int v = threadIdx.x; v < nvars; v += 256) scale[v] = f;
  }
  bad = __syncthreads_or(bad);
  if (threadIdx.x == 0) {
    flag[0] = bad;
    if (found_inf) found_inf[0] = bad;
    if (!bad) {                                     // a skipped step leaves the state where it was
      const double t = state[0] + 1.0, p1 = state[1] * beta1, p2 = state[2] * beta2;
      if (adamw) {                                  // (read by no other rule: two float64 divisions on one thread spared)
        derived[0] = (float)(1.0 / (1.0 - p1));
        derived[1] = (float)(1.0 / (1.0 - p2));
      }
      if (ema_decay > 0.0) {
        double d = ema_decay;
        if (ema_warmup) { const double dw = (1.0 + t) / (10.0 + t); d = dw < d ? dw : d; }
        derived[2] = (float)(1.0 - d);
      }
      state[0] = t; state[1] = p1; state[2] = p2;
    }
  }
}

enum { OPT_RULE_MOMENTUM = 0, OPT_RULE_NESTEROV = 1, OPT_RULE_ADAMW = 2 };
struct OptApplyArgs {
  const OptSeg* segs; const int* block_seg;
  float* w; const float* g; float* a; float* a2; float* e;
  const float* scale; const float* derived; const int* flag;
  float lr, mom, b1, b2, omb1, omb2, eps;   // omb1 = (float)(1 - beta1), omb2 = (float)(1 - beta2): rounded once, on the host
  int vec_ok;                               // every base pointer in use is 16-byte aligned
};
struct OptStepConst { float sc, decay, c1, c2, om; };

// One element; the vector and the scalar path both run exactly this, one rounding per operator in the order written.
template <int RULE, bool EMA>
__device__ __forceinline__ void opt_update(const OptApplyArgs& p, const OptStepConst& k, float& w, float g, float& a, float& a2,
                                           float& e) {
  const float gc = g * k.sc;
  if (RULE == OPT_RULE_ADAMW) {
    a = p.b1 * a + p.omb1 * gc;
    a2 = p.b2 * a2 + p.omb2 * (gc * gc);
    float u = (a * k.c1) / (sqrtf(a2 * k.c2) + p.eps);
    if (k.decay != 0.f) u = u + k.decay * w;        // decoupled: on the update, not on the gradient
    w = w - p.lr * u;
  } else {
    a = p.mom * a + gc;
    if (RULE == OPT_RULE_NESTEROV) w = w - p.lr * (gc + p.mom * a);
    else w = w - p.lr * a;
  }
  if (EMA) e = e + k.om * (w - e);                   // on the value just written
}

template <int RULE, bool EMA>
__device__ __forceinline__ void opt_update_at(const OptApplyArgs& p, const OptStepConst& k, long at) {   // the scalar path's element
  float wi = p.w[at], ai = p.a[at], mi = RULE == OPT_RULE_ADAMW ? p.a2[at] : 0.f, ei = EMA ? p.e[at] : 0.f;
  opt_update<RULE, EMA>(p, k, wi, p.g[at], ai, mi, ei);
  p.w[at] = wi; p.a[at] = ai;
  if (RULE == OPT_RULE_ADAMW) p.a2[at] = mi;
  if (EMA) p.e[at] = ei;
}

template <int RULE, bool EMA>
__global__ __launch_bounds__(256) void opt_apply_opt_kernel(const OptApplyArgs p) {
  if (p.flag[0]) return;   // overflowed step: skipped, in all five buffers
  const int v = p.block_seg[blockIdx.x];
  const OptSeg s = p.segs[v];
  const int lb = blockIdx.x - s.first_block;
  OptStepConst k;
  k.sc = p.scale[v]; k.decay = s.decay;
  k.c1 = RULE == OPT_RULE_ADAMW ? p.derived[0] : 1.f;
  k.c2 = RULE == OPT_RULE_ADAMW ? p.derived[1] : 1.f;
  k.om = EMA ? p.derived[2] : 0.f;
  const long stride = (long)s.nblocks * 256;
  if (p.vec_ok && (s.off & 3) == 0) {
    // 16-byte vectors, never past the segment's end.  A block keeps pass 1's elements -- the 256-element chunks lb*256 + k*stride --
    // so the gradient it wrote there (and the w this pass leaves for the next step's pass 1) is met in its own XCD's L2: with
    // another assignment pass 1 behind this pass took 21.5 us instead of 11.9 on SqueezeDet's table.  Wave `sub` of the block
    // takes the chunks k = sub, sub + 4, ...: one KiB per wave, array and trip.
    const int sub = threadIdx.x >> 6, lane4 = (threadIdx.x & 63) << 2;
    for (long base = (long)lb * 256 + (long)sub * stride; base < s.count; base += 4 * stride) {
      const long i0 = base + lane4;
      if (i0 + 3 >= s.count) {                      // the segment's last 1 .. 3 elements (or none)
        for (long i = i0; i < s.count; ++i) opt_update_at<RULE, EMA>(p, k, s.off + i);
        continue;
      }
      const long at = s.off + i0;
      f32x4 w4 = *reinterpret_cast<const f32x4*>(p.w + at), a4 = *reinterpret_cast<const f32x4*>(p.a + at), m4 = {0.f, 0.f, 0.f, 0.f},
            e4 = {0.f, 0.f, 0.f, 0.f};
      const f32x4 g4 = *reinterpret_cast<const f32x4*>(p.g + at);
      if (RULE == OPT_RULE_ADAMW) m4 = *reinterpret_cast<const f32x4*>(p.a2 + at);
      if (EMA) e4 = *reinterpret_cast<const f32x4*>(p.e + at);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float wj = w4[j], aj = a4[j], mj = m4[j], ej = e4[j];
        opt_update<RULE, EMA>(p, k, wj, g4[j], aj, mj, ej);
        w4[j] = wj; a4[j] = aj; m4[j] = mj; e4[j] = ej;
      }
      *reinterpret_cast<f32x4*>(p.w + at) = w4;
      *reinterpret_cast<f32x4*>(p.a + at) = a4;
      if (RULE == OPT_RULE_ADAMW) *reinterpret_cast<f32x4*>(p.a2 + at) = m4;
      if (EMA) *reinterpret_cast<f32x4*>(p.e + at) = e4;
    }
    return;
  }
  for (long i = (long)lb * 256 + threadIdx.x; i < s.count; i += stride) opt_update_at<RULE, EMA>(p, k, s.off + i);   // odd offsets, unaligned bases
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

static int loss_fwd_bwd_impl(const void* preds, const float* anchors, const float* input_mask,
                             const float* box_delta_input, const float* box_input, const float* labels,
                             float* dpreds, float* ious, float* losses3, float* workspace, int batch, int gh, int gw,
                             int apg, int classes, float img_w, float img_h, float exp_thresh, float epsilon,
                             float coef_class, float coef_conf_pos, float coef_conf_neg, float coef_bbox,
                             float num_objects, const float* num_objects_dev, int global_batch, sqdet_stream_t stream,
                             void* g16 = nullptr, float gscale = 1.f, const LossOpt* opt = nullptr);

extern "C" int sqdet_loss_fwd_bwd_mixed(const void* preds_f16, const float* anchors, const float* input_mask,
                                        const float* box_delta_input, const float* box_input, const float* labels,
                                        float* dpreds, void* dpreds_scaled_f16, float loss_scale, float* ious, float* losses3,
                                        float* workspace, int batch, int gh, int gw, int apg, int classes, float img_w,
                                        float img_h, float exp_thresh, float epsilon, float coef_class, float coef_conf_pos,
                                        float coef_conf_neg, float coef_bbox, float num_objects, const float* num_objects_dev,
                                        int global_batch, sqdet_stream_t stream) {
  SQDET_REQUIRE(dpreds_scaled_f16 && loss_scale > 0.f, "loss_fwd_bwd_mixed: bad arguments");
  return loss_fwd_bwd_impl(preds_f16, anchors, input_mask, box_delta_input, box_input, labels, dpreds, ious, losses3, workspace,
                           batch, gh, gw, apg, classes, img_w, img_h, exp_thresh, epsilon, coef_class, coef_conf_pos,
                           coef_conf_neg, coef_bbox, num_objects_dev ? 1.0f : num_objects, num_objects_dev, global_batch, stream,
                           dpreds_scaled_f16, loss_scale);
}

extern "C" int sqdet_loss_fwd_bwd_dev(const float* preds, const float* anchors, const float* input_mask,
                                      const float* box_delta_input, const float* box_input, const float* labels,
                                      float* dpreds, float* ious, float* losses3, float* workspace, int batch, int gh, int gw,
                                      int apg, int classes, float img_w, float img_h, float exp_thresh, float epsilon,
                                      float coef_class, float coef_conf_pos, float coef_conf_neg, float coef_bbox,
                                      const float* num_objects_dev, int global_batch, sqdet_stream_t stream) {
  SQDET_REQUIRE(num_objects_dev, "loss_fwd_bwd_dev: null num_objects");
  return loss_fwd_bwd_impl(preds, anchors, input_mask, box_delta_input, box_input, labels, dpreds, ious, losses3, workspace,
                           batch, gh, gw, apg, classes, img_w, img_h, exp_thresh, epsilon, coef_class, coef_conf_pos,
                           coef_conf_neg, coef_bbox, 1.0f, num_objects_dev, global_batch, stream);
}

extern "C" int sqdet_loss_fwd_bwd(const float* preds, const float* anchors, const float* input_mask,
                                  const float* box_delta_input, const float* box_input, const float* labels,
                                  float* dpreds, float* ious, float* losses3, float* workspace, int batch, int gh, int gw,
                                  int apg, int classes, float img_w, float img_h, float exp_thresh, float epsilon,
                                  float coef_class, float coef_conf_pos, float coef_conf_neg, float coef_bbox,
                                  float num_objects, int global_batch, sqdet_stream_t stream) {
  return loss_fwd_bwd_impl(preds, anchors, input_mask, box_delta_input, box_input, labels, dpreds, ious, losses3, workspace,
                           batch, gh, gw, apg, classes, img_w, img_h, exp_thresh, epsilon, coef_class, coef_conf_pos,
                           coef_conf_neg, coef_bbox, num_objects, nullptr, global_batch, stream);
}

static int loss_fwd_bwd_impl(const void* preds, const float* anchors, const float* input_mask,
                                  const float* box_delta_input, const float* box_input, const float* labels,
                                  float* dpreds, float* ious, float* losses3, float* workspace, int batch, int gh, int gw,
                                  int apg, int classes, float img_w, float img_h, float exp_thresh, float epsilon,
                                  float coef_class, float coef_conf_pos, float coef_conf_neg, float coef_bbox,
                                  float num_objects, const float* num_objects_dev, int global_batch, sqdet_stream_t stream,
                                  void* g16, float gscale, const LossOpt* opt) {
  SQDET_REQUIRE(preds && anchors && input_mask && box_delta_input && box_input && labels && dpreds && ious && losses3 &&
                    workspace, "loss_fwd_bwd: null pointer");
  SQDET_REQUIRE(batch > 0 && gh > 0 && gw > 0 && apg > 0 && classes > 0 && num_objects > 0.f, "loss_fwd_bwd: bad arguments");
  SQDET_REQUIRE(global_batch <= 0 || global_batch >= batch, "loss_fwd_bwd: global_batch smaller than batch");
  LossArgs a;
  a.preds = preds; a.anchors = anchors; a.mask = input_mask; a.delta_in = box_delta_input; a.box_in = box_input;
  a.labels = labels; a.dpreds = dpreds; a.ious = ious; a.partial = workspace;
  a.g16 = static_cast<f16*>(g16); a.gscale = gscale; a.losses3 = losses3;
  a.B = batch; a.Bmean = global_batch > 0 ? global_batch : batch; a.cells = gh * gw; a.K = apg; a.C = classes;
  a.w1 = img_w - 1.0f; a.h1 = img_h - 1.0f; a.thr = exp_thresh; a.slope = (float)exp((double)exp_thresh); a.eps = epsilon;
  a.coef_class = coef_class; a.coef_pos = coef_conf_pos; a.coef_neg = coef_conf_neg; a.coef_bbox = coef_bbox;
  a.num_obj = num_objects;
  a.num_obj_dev = num_objects_dev;
  const long total = (long)batch * gh * gw * apg;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 512) blocks = 512;
  hipStream_t st = as_stream(stream);
  if (opt && g16) hipLaunchKernelGGL(loss_opt_kernel<f16>, dim3(blocks), dim3(256), 0, st, a, *opt);
  else if (opt) hipLaunchKernelGGL(loss_opt_kernel<float>, dim3(blocks), dim3(256), 0, st, a, *opt);
  else if (g16) hipLaunchKernelGGL(loss_kernel<f16>, dim3(blocks), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(loss_kernel<float>, dim3(blocks), dim3(256), 0, st, a);
  SQDET_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, st, workspace, losses3, blocks);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

// The loss with options: the defaults ARE the three entry points above; anything else is loss_opt_kernel.
extern "C" int sqdet_loss_fwd_bwd_opt(const void* preds, int preds_dtype, const float* anchors, const float* input_mask,
                                      const float* box_delta_input, const float* box_input, const float* labels,
                                      float* dpreds, void* dpreds_scaled_f16, float loss_scale, float* ious, float* losses3,
                                      float* workspace, int batch, int gh, int gw, int apg, int classes, float img_w,
                                      float img_h, float exp_thresh, float epsilon, float coef_class, float coef_conf_pos,
                                      float coef_conf_neg, float coef_bbox, float num_objects, const float* num_objects_dev,
                                      int global_batch, const sqdet_loss_options_t* opt, sqdet_stream_t stream) {
  SQDET_REQUIRE(opt, "loss_fwd_bwd_opt: null options");
  SQDET_REQUIRE(opt->box_loss >= SQDET_BOX_LOSS_DELTA_L2 && opt->box_loss <= SQDET_BOX_LOSS_CIOU, "loss_fwd_bwd_opt: box_loss %d is not one of 0..4", opt->box_loss);
  SQDET_REQUIRE(opt->focal_gamma >= 0.f && opt->focal_gamma < INFINITY, "loss_fwd_bwd_opt: focal_gamma must be finite and >= 0");
  SQDET_REQUIRE(preds_dtype == SQDET_F32 || preds_dtype == SQDET_F16, "loss_fwd_bwd_opt: bad dtype");
  const bool mixed = preds_dtype == SQDET_F16;
  SQDET_REQUIRE(!mixed || (dpreds_scaled_f16 && loss_scale > 0.f), "loss_fwd_bwd_opt: float16 preds need dpreds_scaled_f16 and a loss scale");
  if (opt->box_loss == SQDET_BOX_LOSS_DELTA_L2 && opt->focal_gamma == 0.f) {
    if (mixed)
      return sqdet_loss_fwd_bwd_mixed(preds, anchors, input_mask, box_delta_input, box_input, labels, dpreds, dpreds_scaled_f16,
                                      loss_scale, ious, losses3, workspace, batch, gh, gw, apg, classes, img_w, img_h, exp_thresh,
                                      epsilon, coef_class, coef_conf_pos, coef_conf_neg, coef_bbox, num_objects, num_objects_dev,
                                      global_batch, stream);
    if (num_objects_dev)
      return sqdet_loss_fwd_bwd_dev((const float*)preds, anchors, input_mask, box_delta_input, box_input, labels, dpreds, ious,
                                    losses3, workspace, batch, gh, gw, apg, classes, img_w, img_h, exp_thresh, epsilon, coef_class,
                                    coef_conf_pos, coef_conf_neg, coef_bbox, num_objects_dev, global_batch, stream);
    return sqdet_loss_fwd_bwd((const float*)preds, anchors, input_mask, box_delta_input, box_input, labels, dpreds, ious, losses3,
                              workspace, batch, gh, gw, apg, classes, img_w, img_h, exp_thresh, epsilon, coef_class, coef_conf_pos,
                              coef_conf_neg, coef_bbox, num_objects, global_batch, stream);
  }
  const LossOpt o = {opt->box_loss, opt->focal_gamma};
  return loss_fwd_bwd_impl(preds, anchors, input_mask, box_delta_input, box_input, labels, dpreds, ious, losses3, workspace,
                           batch, gh, gw, apg, classes, img_w, img_h, exp_thresh, epsilon, coef_class, coef_conf_pos,
                           coef_conf_neg, coef_bbox, num_objects_dev ? 1.0f : num_objects, num_objects_dev, global_batch, stream,
                           mixed ? dpreds_scaled_f16 : nullptr, mixed ? loss_scale : 1.f, &o);
}

extern "C" size_t sqdet_loss_workspace_bytes(void) { return (4 * 512 + 4) * sizeof(float); }

// Distillation: distill_kernel onto the dpreds the loss launch wrote, then loss_finish_kernel into distill3.
extern "C" size_t sqdet_distill_workspace_bytes(void) { return (4 * 512 + 4) * sizeof(float); }

extern "C" int sqdet_distill_fwd_bwd(const void* preds, int preds_dtype, const void* teacher_preds, int teacher_dtype,
                                     float* dpreds_inout, void* dpreds_scaled_f16, float loss_scale, float* distill3,
                                     float* workspace, int batch, int gh, int gw, int apg, int classes, int global_batch,
                                     const sqdet_distill_options_t* opt, sqdet_stream_t stream) {
  SQDET_REQUIRE(preds && teacher_preds && dpreds_inout && distill3 && workspace && opt, "distill_fwd_bwd: null pointer");
  SQDET_REQUIRE(batch > 0 && gh > 0 && gw > 0 && apg > 0 && classes > 0, "distill_fwd_bwd: bad arguments");
  SQDET_REQUIRE(global_batch <= 0 || global_batch >= batch, "distill_fwd_bwd: global_batch smaller than batch");
  SQDET_REQUIRE(opt->temperature > 0.f && opt->temperature < INFINITY, "distill_fwd_bwd: temperature must be finite and > 0");
  const float coefs[3] = {opt->class_coef, opt->conf_coef, opt->bbox_coef};
  for (int i = 0; i < 3; ++i)
    SQDET_REQUIRE(coefs[i] >= 0.f && coefs[i] < INFINITY, "distill_fwd_bwd: coefficients must be finite and >= 0");
  SQDET_REQUIRE(coefs[0] > 0.f || coefs[1] > 0.f || coefs[2] > 0.f, "distill_fwd_bwd: all three coefficients are zero");
  SQDET_REQUIRE(opt->conf_floor >= 0.f && opt->conf_floor <= 1.f, "distill_fwd_bwd: conf_floor must lie in [0, 1]");
  SQDET_REQUIRE((preds_dtype == SQDET_F32 || preds_dtype == SQDET_F16) && (teacher_dtype == SQDET_F32 || teacher_dtype == SQDET_F16),
                "distill_fwd_bwd: bad dtype");
  const bool half = preds_dtype == SQDET_F16, thalf = teacher_dtype == SQDET_F16;
  SQDET_REQUIRE(!half || (dpreds_scaled_f16 && loss_scale > 0.f), "distill_fwd_bwd: float16 preds need dpreds_scaled_f16 and a loss scale");
  DistillArgs a;
  a.preds = preds; a.teacher = teacher_preds; a.dpreds = dpreds_inout; a.partial = workspace;
  a.g16 = half ? static_cast<f16*>(dpreds_scaled_f16) : nullptr; a.gscale = half ? loss_scale : 1.f;
  a.B = batch; a.cells = gh * gw; a.K = apg; a.C = classes;
  a.Bg = (float)(global_batch > 0 ? global_batch : batch);
  a.BgA = a.Bg * (float)(gh * gw * apg);
  a.T = opt->temperature; a.c_cls = opt->class_coef; a.c_conf = opt->conf_coef; a.c_box = opt->bbox_coef; a.floor = opt->conf_floor;
  const long total = (long)batch * gh * gw * apg;
  int blocks = (int)((total + 255) / 256);
  if (blocks > 512) blocks = 512;
  hipStream_t st = as_stream(stream);
  if (half && thalf) hipLaunchKernelGGL((distill_kernel<f16, f16>), dim3(blocks), dim3(256), 0, st, a);
  else if (half) hipLaunchKernelGGL((distill_kernel<f16, float>), dim3(blocks), dim3(256), 0, st, a);
  else if (thalf) hipLaunchKernelGGL((distill_kernel<float, f16>), dim3(blocks), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((distill_kernel<float, float>), dim3(blocks), dim3(256), 0, st, a);
  SQDET_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(loss_finish_kernel, dim3(1), dim3(256), 0, st, workspace, distill3, blocks);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

// ---- optimizer: host-side segment table lives in a small opaque object ----
struct sqdet_optimizer {
  std::vector<OptSeg> segs;
  std::vector<int> block_seg;
  int nblocks = 0;
};

extern "C" int sqdet_optimizer_create(sqdet_optimizer** out, const long* offsets, const long* counts, const float* decays,
                                      int nvars) {
  SQDET_REQUIRE(out && offsets && counts && decays && nvars > 0, "optimizer_create: bad arguments");
  sqdet_optimizer* o = new sqdet_optimizer();
  for (int v = 0; v < nvars; ++v) {
    OptSeg s;
    s.off = offsets[v]; s.count = counts[v]; s.decay = decays[v];
    long nb = (counts[v] + 256 * 8 - 1) / (256 * 8);
    if (nb < 1) nb = 1;
    if (nb > 64) nb = 64;
    s.first_block = o->nblocks; s.nblocks = (int)nb;
    o->nblocks += (int)nb;
    for (long b = 0; b < nb; ++b) o->block_seg.push_back(v);
    o->segs.push_back(s);
  }
  *out = o;
  return SQDET_OK;
}

extern "C" void sqdet_optimizer_destroy(sqdet_optimizer* o) { delete o; }

extern "C" size_t sqdet_optimizer_workspace_bytes(const sqdet_optimizer* o) {
  if (!o) return 0;
  // segs | block_seg | partial (double) | scale
  size_t b = o->segs.size() * sizeof(OptSeg);
  b = (b + 255) / 256 * 256 + o->block_seg.size() * sizeof(int);
  b = (b + 255) / 256 * 256 + (size_t)o->nblocks * sizeof(double);
  b = (b + 255) / 256 * 256 + o->segs.size() * sizeof(float);
  return b + 256;
}

extern "C" int sqdet_optimizer_step(sqdet_optimizer* o, float* params, float* grads, float* accum, void* workspace,
                                    float lr, float momentum, float max_grad_norm, float grad_scale, int32_t* found_inf,
                                    sqdet_stream_t stream) {
  SQDET_REQUIRE(o && params && grads && accum && workspace, "optimizer_step: null pointer");
  hipStream_t st = as_stream(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  size_t off = 0;
  OptSeg* d_segs = reinterpret_cast<OptSeg*>(ws + off);
  off = (off + o->segs.size() * sizeof(OptSeg) + 255) / 256 * 256;
  int* d_bs = reinterpret_cast<int*>(ws + off);
  off = (off + o->block_seg.size() * sizeof(int) + 255) / 256 * 256;
  double* d_part = reinterpret_cast<double*>(ws + off);
  off = (off + (size_t)o->nblocks * sizeof(double) + 255) / 256 * 256;
  float* d_scale = reinterpret_cast<float*>(ws + off);
  SQDET_CHECK_HIP(hipMemcpyAsync(d_segs, o->segs.data(), o->segs.size() * sizeof(OptSeg), hipMemcpyHostToDevice, st));
  SQDET_CHECK_HIP(hipMemcpyAsync(d_bs, o->block_seg.data(), o->block_seg.size() * sizeof(int), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(opt_sumsq_kernel, dim3(o->nblocks), dim3(256), 0, st, d_segs, d_bs, params, grads, d_part, grad_scale);
  SQDET_CHECK_HIP(hipGetLastError());
  int* d_flag = reinterpret_cast<int*>(d_scale + o->segs.size());
  hipLaunchKernelGGL(opt_norm_kernel, dim3(1), dim3(256), 0, st, d_segs, d_part, d_scale, (int)o->segs.size(), max_grad_norm,
                     d_flag, found_inf);
  SQDET_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(opt_apply_kernel, dim3(o->nblocks), dim3(256), 0, st, d_segs, d_bs, params, grads, accum, d_scale, lr,
                     momentum, d_flag);
  SQDET_CHECK_HIP(hipGetLastError());
  return SQDET_OK;
}

template <int RULE>
static void launch_opt_apply(bool ema, int nblocks, hipStream_t st, const OptApplyArgs& p) {
  if (ema) hipLaunchKernelGGL((opt_apply_opt_kernel<RULE, true>), dim3(nblocks), dim3(256), 0, st, p);
  else hipLaunchKernelGGL((opt_apply_opt_kernel<RULE, false>), dim3(nblocks), dim3(256), 0, st, p);
}

// (workspace: sqdet_optimizer_step's layout; the three derived float32 scalars follow its flag word, inside the 256 spare bytes)
extern "C" int sqdet_optimizer_step_opt(sqdet_optimizer* o, float* params, float* grads, float* accum, float* accum2, float* ema,
                                        double* state, void* workspace, float lr, float max_grad_norm, float grad_scale,
                                        const sqdet_optimizer_options_t* opt, int32_t* found_inf, sqdet_stream_t stream) {
  SQDET_REQUIRE(o && params && grads && accum && state && workspace && opt, "optimizer_step_opt: null pointer");
  SQDET_REQUIRE(opt->rule >= OPT_RULE_MOMENTUM && opt->rule <= OPT_RULE_ADAMW, "optimizer_step_opt: rule must be 0 (momentum), 1 (nesterov) or 2 (adamw)");
  SQDET_REQUIRE(opt->clip == 0 || opt->clip == 1, "optimizer_step_opt: clip must be 0 (per variable) or 1 (global)");
  SQDET_REQUIRE(opt->momentum >= 0.f && opt->momentum < 1.f, "optimizer_step_opt: momentum must lie in [0, 1)");
  SQDET_REQUIRE(opt->beta1 >= 0.f && opt->beta1 < 1.f && opt->beta2 >= 0.f && opt->beta2 < 1.f, "optimizer_step_opt: beta1 and beta2 must lie in [0, 1)");
  SQDET_REQUIRE(opt->eps > 0.f && opt->eps <= 3.0e38f, "optimizer_step_opt: eps must be finite and positive");
  SQDET_REQUIRE(opt->ema_decay >= 0.0 && opt->ema_decay < 1.0, "optimizer_step_opt: ema_decay must lie in [0, 1)");
  SQDET_REQUIRE(opt->rule != OPT_RULE_ADAMW || accum2, "optimizer_step_opt: adamw needs accum2");
  SQDET_REQUIRE(!(opt->ema_decay > 0.0) || ema, "optimizer_step_opt: ema_decay > 0 needs the ema buffer");
  for (const OptSeg& s : o->segs)
    SQDET_REQUIRE(s.decay >= 0.f && s.decay <= 3.0e38f, "optimizer_step_opt: a variable's decay must be finite and >= 0");
  const bool adamw = opt->rule == OPT_RULE_ADAMW, use_ema = opt->ema_decay > 0.0;
  hipStream_t st = as_stream(stream);
  char* ws = reinterpret_cast<char*>(workspace);
  size_t off = 0;
  OptSeg* d_segs = reinterpret_cast<OptSeg*>(ws + off);
  off = (off + o->segs.size() * sizeof(OptSeg) + 255) / 256 * 256;
  int* d_bs = reinterpret_cast<int*>(ws + off);
  off = (off + o->block_seg.size() * sizeof(int) + 255) / 256 * 256;
  double* d_part = reinterpret_cast<double*>(ws + off);
  off = (off + (size_t)o->nblocks * sizeof(double) + 255) / 256 * 256;
  float* d_scale = reinterpret_cast<float*>(ws + off);
  int* d_flag = reinterpret_cast<int*>(d_scale + o->segs.size());
  float* d_derived = reinterpret_cast<float*>(d_flag + 1);
  SQDET_CHECK_HIP(hipMemcpyAsync(d_segs, o->segs.data(), o->segs.size() * sizeof(OptSeg), hipMemcpyHostToDevice, st));
  SQDET_CHECK_HIP(hipMemcpyAsync(d_bs, o->block_seg.data(), o->block_seg.size() * sizeof(int), hipMemcpyHostToDevice, st));
  if (adamw)
    hipLaunchKernelGGL((opt_sumsq_opt_kernel<false>), dim3(o->nblocks), dim3(256), 0, st, d_segs, d_bs, params, grads, d_part, grad_scale);
  else
    hipLaunchKernelGGL((opt_sumsq_opt_kernel<true>), dim3(o->nblocks), dim3(256), 0, st, d_segs, d_bs, params, grads, d_part, grad_scale);
  SQDET_CHECK_HIP(hipGetLastError());
  hipLaunchKernelGGL(opt_norm_opt_kernel, dim3(1), dim3(256), 0, st, d_segs, d_part, d_scale, (int)o->segs.size(), max_grad_norm,
                     opt->clip, adamw ? 1 : 0, (double)opt->beta1, (double)opt->beta2, use_ema ? opt->ema_decay : 0.0, opt->ema_warmup != 0, state,
                     d_derived, d_flag, found_inf);
  SQDET_CHECK_HIP(hipGetLastError());
  OptApplyArgs p;
  p.segs = d_segs; p.block_seg = d_bs;
  p.w = params; p.g = grads; p.a = accum; p.a2 = adamw ? accum2 : nullptr; p.e = use_ema ? ema : nullptr;
  p.scale = d_scale; p.derived = d_derived; p.flag = d_flag;
  p.lr = lr; p.mom = opt->momentum; p.b1 = opt->beta1; p.b2 = opt->beta2; p.eps = opt->eps;
  p.omb1 = (float)(1.0 - (double)opt->beta1); p.omb2 = (float)(1.0 - (double)opt->beta2);
  uintptr_t bits = reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grads) | reinterpret_cast<uintptr_t>(accum);
  if (adamw) bits |= reinterpret_cast<uintptr_t>(accum2);
  if (use_ema) bits |= reinterpret_cast<uintptr_t>(ema);
  p.vec_ok = (bits & 15) == 0;
  if (opt->rule == OPT_RULE_MOMENTUM) launch_opt_apply<OPT_RULE_MOMENTUM>(use_ema, o->nblocks, st, p);
  else if (opt->rule == OPT_RULE_NESTEROV) launch_opt_apply<OPT_RULE_NESTEROV>(use_ema, o->nblocks, st, p);
  else launch_opt_apply<OPT_RULE_ADAMW>(use_ema, o->nblocks, st, p);
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
