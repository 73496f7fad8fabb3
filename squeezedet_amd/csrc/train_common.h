// What the training step's translation units share (train.hip's element-wise kernels, loss.hip): compiled with
// -ffp-contract=off in each.
#pragma once
#include "common.h"

namespace sqdet {

// (D)(v * scale), the product formed on its own.  Left to itself hipcc fuses a float32 multiply and the conversion to float16
// into v_fma_mixlo_f16(v, scale, +0), and (-0) + (+0) = +0: the sign of a zero product was lost -- on two of convert_scale's four
// lanes (the other two go through v_pk_mul_f32 + v_cvt_pk_f16_f32 and kept it) and in some of the loss kernel's stores.
template <typename D>
__device__ __forceinline__ D scaled_to(float v, float scale) {
  float p = v * scale;
  asm volatile("" : "+v"(p));
  return (D)p;
}

}  // namespace sqdet
