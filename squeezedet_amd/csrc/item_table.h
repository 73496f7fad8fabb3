// The item tables of the training step's "many" launches (pack_many_kernel in train.hip, the fold_bn_bwd_*_many kernels in
// bn.hip, slab_reduce_many_kernel in wgrad.hip): one launch serves many items, every item owns a range of consecutive
// workgroups, and the ranges follow each other from workgroup 0 in table order.  The host hands the ranges out with a
// BlockCursor while it fills the table; a workgroup finds its item with item_of_block and then runs the same __device__ body
// as the per-item kernel, on its range-local block index -- which is why a "many" launch gives the per-item entry's bits.
#pragma once
#include "common.h"

namespace sqdet {

// Hands out consecutive workgroup ranges: take(nblocks) returns the range's first workgroup; total is the grid so far.
struct BlockCursor {
  unsigned total = 0;
  unsigned take(unsigned nblocks) { total += nblocks; return total - nblocks; }
};

// The last of the n items whose range start (the member First: an item with two launches has two) is <= block.
template <typename Item, unsigned Item::*First>
__device__ __forceinline__ const Item& item_of_block(const Item* __restrict__ items, int n, unsigned block) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (items[mid].*First <= block) lo = mid; else hi = mid - 1;
  }
  return items[lo];
}

}  // namespace sqdet
