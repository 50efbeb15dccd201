// scan_ordered.hpp — launchers of the ordered variants of the one-shot scan
// kernels (implementation: scan_ordered.hip, which compiles the kernels of
// scan_kernels.hip in their ordered mode). Private to csrc/hip.
//
// The ordered kernels live in a translation unit of their own so that the
// default kernels of scan_kernels.hip compile to exactly the code they had
// before there was a second mode: with both instantiations in one module the
// optimizer scheduled the default k_scan5 differently (same registers, same
// scratch, 0.4% slower on the 5-LUT benchmark).
#pragma once

#include <hip/hip_runtime.h>

#include "sbg/common.hpp"

namespace sbg {

enum OrderedScan {
  ORDERED_SCAN3,
  ORDERED_SCAN4,
  ORDERED_SCAN5_ROWS,  // k_scan5<false, ...>: pools without a long row
  ORDERED_SCAN5_WIDE,  // k_scan5<true, ...>
  ORDERED_SCAN4S,
};

// Launches the ordered kernel `which` on `grid` workgroups of SCAN_BLOCK
// threads. scan_args points to a ScanArgs (scan_device.hpp), whose type is
// local to each translation unit and therefore travels as void.
void launch_ordered_scan(OrderedScan which, int grid, hipStream_t stream,
                         const void* scan_args);

// Launches the ordered k_scan7_assign over nhits entries of the Hit7 buffer
// `hits`; ctl is the device DevCtl, whose pool_n holds the pool size.
void launch_ordered_assign7(int grid, hipStream_t stream, const void* hits,
                            unsigned long long nhits, void* ctl, u64 seed);

}  // namespace sbg
