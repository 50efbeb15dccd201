// scan_default.hip — the default-mode module of the one-shot scan kernels:
// the ORD = false instantiations, the kernels that have one variant
// (k_scan2, k_scan7_filter) and their launchers. Ordered mode:
// scan_ordered.hip; why two modules: scan_launch.hpp.

#include "scan_launch.hpp"
#include "scan_strided.hpp"
#include "scan_pairs.hpp"
#include "scan5.hpp"
#include "scan4s.hpp"
#include "scan7_filter.hpp"
#include "scan7_assign.hpp"

namespace sbg {

void launch_scan_default(ScanKernel which, int grid, hipStream_t stream,
                         const ScanArgs& args) {
  void (*kernel)(ScanArgs) = nullptr;
  switch (which) {
    case KERNEL_SCAN2: kernel = k_scan2; break;
    case KERNEL_SCAN3: kernel = k_scan3<false>; break;
    case KERNEL_SCAN4: kernel = k_scan4<false>; break;
    // Wide first: the module then lays its kernels out as the single-file
    // layout did (profiles/hip_layout.md).
    case KERNEL_SCAN5_WIDE: kernel = k_scan5<true, false>; break;
    case KERNEL_SCAN5_ROWS: kernel = k_scan5<false, false>; break;
    case KERNEL_SCAN4S: kernel = k_scan4s<false>; break;
    case KERNEL_SCAN7_FILTER: kernel = k_scan7_filter; break;
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(SCAN_BLOCK), 0, stream, args);
}

void launch_assign7_default(int grid, hipStream_t stream, const Hit7* hits,
                            unsigned long long nhits, DevCtl* ctl, u64 seed) {
  hipLaunchKernelGGL(k_scan7_assign<false>, dim3(grid), dim3(SCAN_BLOCK), 0,
                     stream, hits, nhits, ctl, seed);
}

}  // namespace sbg
