// Shared device helpers of the conv kernels (conv.hip, conv3x3.hip) and of the weight packers (conv.hip, train.hip); their
// host-side launchers are declared in launch.h.
#pragma once
#include "common.h"
#include "launch.h"

namespace sqdet {

template <typename T> struct Tr;
template <> struct Tr<f16> { static constexpr int KG = 8; };
template <> struct Tr<float> { static constexpr int KG = 4; };

template <typename T>
__device__ __forceinline__ void mma16(f32x4& acc, const i32x4& a, const i32x4& b);
template <>
__device__ __forceinline__ void mma16<f16>(f32x4& acc, const i32x4& a, const i32x4& b) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), acc, 0, 0, 0);
}
template <>
__device__ __forceinline__ void mma16<float>(f32x4& acc, const i32x4& a, const i32x4& b) {
  f32x4 af = __builtin_bit_cast(f32x4, a), bf = __builtin_bit_cast(f32x4, b);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[0], bf[0], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[1], bf[1], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[2], bf[2], acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af[3], bf[3], acc, 0, 0, 0);
}

struct ConvArgs {
  const void* x;
  const void* wp;
  const float* bias;
  void* y;
  int N, H, W, Cin, Cout, k, stride, pt, pl, Ho, Wo;
  int P;        // N*Ho*Wo output pixels
  int ntiles;   // ceil(P / (16*MT))
  int nchunk, steps, ngroups;
  int y_cstride, y_coffset, relu;
  // generic kernel only: the input may be a channel slice [x_coffset, x_coffset+Cin) of rows
  // x_cstride channels wide, and the result may be ADDED to y (backward-data of a fire module:
  // d(squeeze) = dgrad_1x1(dY[:, :e1]) + dgrad_3x3(dY[:, e1:])).
  int x_cstride, x_coffset, accum;
  // accum only: the tensor the result is added to when it is NOT y itself (same layout as y; NULL = y).  ResNet50's training forward
  // keeps the shortcut for the backward pass: y = relu(conv(x) + b + res) without a copy of the shortcut first.  Honoured by
  // conv1x1_pipe; every other kernel gets a copy res -> y in front (conv2d_launch_res).
  const void* res;
  // backward-data only: the result is the gradient w.r.t. a ReLU OUTPUT r (same layout as y); it is zeroed where r <= 0 --
  // the ReLU backward of the layer below, taken in this conv's epilogue instead of a separate pass over the tensor
  const void* relu_of;
  // ConvDet only (convdet.hip, float16): when not NULL, the epilogue also writes one float32 SCORE per anchor --
  // det_probs of interpret_output (nn_skeleton.py:150-170, 274-283) computed from the float16-rounded preds it stores --
  // to scores[N, H*W*score_apg]; Cout = score_apg * (score_classes + 5), score_classes == 3
  float* scores;
  int score_apg, score_classes;
};

template <typename T>
__device__ __forceinline__ void store4(T* dst, const f32x4& v);
template <>
__device__ __forceinline__ void store4<f16>(f16* dst, const f32x4& v) {
  f16x4 h = {(f16)v[0], (f16)v[1], (f16)v[2], (f16)v[3]};
  *reinterpret_cast<f16x4*>(dst) = h;
}
template <>
__device__ __forceinline__ void store4<float>(float* dst, const f32x4& v) {
  *reinterpret_cast<f32x4*>(dst) = v;
}

// Stores 4*NT consecutive output channels held by one lane (nt_valid < NT: only the first nt_valid
// 4-channel pieces exist).  fp16 rows go out as 16-byte vectors when the pieces pair up.
template <typename T, int NT>
__device__ __forceinline__ void store_couts(T* dst, const f32x4 (&v)[NT], int nt_valid) {
  if (nt_valid == NT) {
    // 16-byte stores need a 16-byte aligned row segment: even NT (8*NT bytes per lane) and a row
    // stride / channel offset that are multiples of 8 halves -- checked on the address itself.
    if (sizeof(T) == 2 && (NT & 1) == 0 && (reinterpret_cast<uintptr_t>(dst) & 15) == 0) {
#pragma unroll
      for (int t = 0; t + 1 < NT; t += 2) {
        f16x8 h = {(f16)v[t][0], (f16)v[t][1], (f16)v[t][2], (f16)v[t][3],
                   (f16)v[t + 1][0], (f16)v[t + 1][1], (f16)v[t + 1][2], (f16)v[t + 1][3]};
        *reinterpret_cast<f16x8*>(dst + t * 4) = h;
      }
    } else {
#pragma unroll
      for (int t = 0; t < NT; ++t) store4<T>(dst + t * 4, v[t]);
    }
  } else {
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (t < nt_valid) store4<T>(dst + t * 4, v[t]);
  }
}

// ---- weight packing: float32 HWIO -> [group][step][nt][lane][KG] fragments of the conv that will read them ----
// element idx = (group, step=(tap,chunk), n, lane=(i=lane&15, g=lane>>4), e):
//   co = group*16*NT + (i>>2)*4*NT + n*4 + (i&3)      (row i of tile n <-> consecutive output channels per lane)
//   ci = chunk*KC + g*KG + e
struct PackIdx { int tap, ci, co; };

template <typename T>
__device__ __forceinline__ PackIdx pack_index(size_t idx, int nt, int nchunk, int taps) {
  constexpr int KG = Tr<T>::KG;
  constexpr int KC = 4 * KG;
  size_t t = idx;
  const int e = t % KG; t /= KG;
  const int lane = t % 64; t /= 64;
  const int n = t % nt; t /= nt;
  const int step = t % (taps * nchunk); t /= (taps * nchunk);
  const int group = (int)t;
  const int tap = step / nchunk, chunk = step - tap * nchunk;
  const int i = lane & 15, g = lane >> 4;
  return {tap, chunk * KC + g * KG + e, group * 16 * nt + (i >> 2) * 4 * nt + n * 4 + (i & 3)};
}

// The element's value in v (0 in the padding beyond the kernel's channels); returns whether the element exists.
// Forward order: the conv reads taps x kdim input values per output channel.
__device__ __forceinline__ bool pack_fetch_fwd(const float* __restrict__ w, const PackIdx& p, int kdim, int cout, float& v) {
  const bool in = p.co < cout && p.ci < kdim;
  v = in ? w[((size_t)p.tap * kdim + p.ci) * cout + p.co] : 0.f;
  return in;
}

// Backward-data order: dgrad(dy)[ci] = sum_{tap,co} W[k-1-ty][k-1-tx][ci][co] * dy@tap[co] is a forward conv with kernel
// W'[ty][tx][co][ci], so its output channel p.co is an original cin and its input channel p.ci an original cout.
__device__ __forceinline__ bool pack_fetch_bwd(const float* __restrict__ w, const PackIdx& p, int k, int cin, int cout, float& v) {
  const int ty = p.tap / k, tx = p.tap - ty * k;
  const bool in = p.co < cin && p.ci < cout;
  v = in ? w[(((size_t)(k - 1 - ty) * k + (k - 1 - tx)) * cin + p.co) * cout + p.ci] : 0.f;
  return in;
}

}  // namespace sqdet
