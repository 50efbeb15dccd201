// scan7_assign.hpp — second half of the 7-LUT scan: the function assignment
// k_scan7_assign over the hits of k_scan7_filter (scan7_filter.hpp).
// Included by the kernel modules only (scan_launch.hpp).
#pragma once

#include "scan_device.hpp"

namespace sbg {
namespace {

// ---------------------------------------------------------------------------
// K4b — 7-LUT function assignment over filtered hits: one thread per
// (hit, ordering); each runs the middle-function sweep + outer 2-coloring
// (replacing the reference's 70 x 256 x 256 brute force, lut.c:416-484).
//
// ORD: the filter appends its hits in no particular order, so an item that
// solves lowers ctl->best with the rank of its hit's combination (computed
// here from the hit's gate ids, dev_rank7; Hit7 keeps its size) and the
// thread goes on: a later item of its own may belong to a lower rank. Items
// of hits that rank above the best known are skipped. The pool size that
// the rank needs comes in ctl->pool_n, so both variants keep one signature.
// ---------------------------------------------------------------------------
template <bool ORD>
__global__ void __launch_bounds__(SCAN_BLOCK) k_scan7_assign(
    const Hit7* hits, unsigned long long nhits, DevCtl* ctl, u64 seed) {
  // One thread per (hit, ordering, fm-octant): the 256-middle-function
  // sweep splits across 8 threads (disjoint 32-function slices of the
  // same shuffled order), which bounds the divergent tail of exhaustive
  // items at ~32 colorings and feeds the GPU 8x more parallel slack.
  constexpr int FM_SLICE = 256 / static_cast<int>(FM_SPLIT);
  const u64 nitems = nhits * LUT7_NUM_ORDERINGS * FM_SPLIT;
  const u64 stride = static_cast<u64>(gridDim.x) * blockDim.x;
  int tick = 0;
  for (u64 item = blockIdx.x * static_cast<u64>(blockDim.x) + threadIdx.x;
       item < nitems; item += stride) {
    if constexpr (!ORD) {
      if (((tick++) & 3) == 0 && dev_abort(ctl)) return;
    }
    const u64 base_item = item / FM_SPLIT;
    const int oct = static_cast<int>(item % FM_SPLIT);
    const Hit7& h = hits[base_item / LUT7_NUM_ORDERINGS];
    u64 rank = 0;
    if constexpr (ORD) {
      rank = static_cast<u64>(
          dev_rank7(h.nums, static_cast<int>(ctl->pool_n)));
      if (rank >= dev_best(ctl)) continue;
    }
    int oidx = static_cast<int>(base_item % LUT7_NUM_ORDERINGS);
    u8 ord[7];
    lut7_ordering(oidx, ord);
    u8 fo, fm, fi;
    // rnd keyed by (hit, ordering) so the 8 octants partition the same
    // shuffled middle-function order disjointly.
    if (lut7_solve_ordering(h.p1, h.p0, ord, scan_rnd(seed, base_item), &fo,
                            &fm, &fi, oct * FM_SLICE, FM_SLICE)) {
      if constexpr (ORD) {
        dev_lower_best(ctl, rank);
        continue;
      }
      u16 res[10];
      res[0] = fo;
      res[1] = fm;
      res[2] = fi;
      for (int j = 0; j < 7; j++) res[3 + j] = h.nums[ord[j]];
      dev_publish(ctl, res);
      return;
    }
  }
}

}  // namespace
}  // namespace sbg
