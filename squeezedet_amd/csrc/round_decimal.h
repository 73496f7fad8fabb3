// Decimal rounding as Python's '%.<d>f' does it, for the kernels whose output is compared with text a host program prints
// (det_table.h: the detection files' '%.2f' / '{:.1f}' / '%.3f'; draw.hip: the '%.2f' of a label).  Build with -ffp-contract=off.
#pragma once
#include "common.h"

namespace sqdet {

// The integer v * scale rounded half-to-even on the EXACT product (scale = 10^d): fma gives the rounding error of the
// product, which decides a tie of the rounded product.
__device__ __forceinline__ double round_decimal_units(double v, double scale) {
  const double p = v * scale;
  const double e = __builtin_fma(v, scale, -p);
  double k = __builtin_rint(p);
  if (__builtin_fabs(p - k) == 0.5 && e != 0) k = e > 0 ? __builtin_floor(p) + 1.0 : __builtin_floor(p);
  return k;
}

// The double nearest to the decimal that '%.<d>f' prints for v.
__device__ __forceinline__ double round_decimal(double v, double scale) { return round_decimal_units(v, scale) / scale; }

}  // namespace sqdet
