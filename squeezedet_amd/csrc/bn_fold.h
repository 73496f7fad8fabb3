// The frozen batch norm's fold expressions, shared by fold_bn_kernel (bn.hip) and pack_many_kernel (train.hip), which must
// agree bit for bit.  bn_fold_bias is a multiply followed by an add: it rounds twice only where the compiler may not contract
// it into one fused multiply-add.  So this header is for translation units built with -ffp-contract=off -- bn.hip and
// train.hip are, conv.hip and wgrad.hip are not -- and no other file may include it.
#pragma once
#include "common.h"

namespace sqdet {

__device__ __forceinline__ float bn_fold_scale(float gamma, float var, float eps) { return gamma / sqrtf(var + eps); }

// channel c's folded bias; inv = bn_fold_scale of that channel, cbias may be NULL (a conv without a bias)
__device__ __forceinline__ float bn_fold_bias(const float* cbias, const float* mean, const float* beta, int c, float inv) {
  return ((cbias ? cbias[c] : 0.f) - mean[c]) * inv + beta[c];
}

}  // namespace sqdet
