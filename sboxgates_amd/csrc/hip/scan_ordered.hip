// scan_ordered.hip — the ordered-mode module (ScanRequest::ordered) of the
// one-shot scan kernels: the ORD = true instantiations and their launchers.
// Default mode: scan_default.hip; why two modules: scan_launch.hpp.

#include "scan_launch.hpp"
#include "scan_strided.hpp"
#include "scan5.hpp"
#include "scan4s.hpp"
#include "scan7_assign.hpp"

namespace sbg {

void launch_scan_ordered(ScanKernel which, int grid, hipStream_t stream,
                         const ScanArgs& args) {
  void (*kernel)(ScanArgs) = nullptr;
  switch (which) {
    case KERNEL_SCAN2:
    case KERNEL_SCAN7_FILTER:  // one variant, in the default module
      launch_scan_default(which, grid, stream, args);
      return;
    case KERNEL_SCAN3: kernel = k_scan3<true>; break;
    case KERNEL_SCAN4: kernel = k_scan4<true>; break;
    case KERNEL_SCAN5_ROWS: kernel = k_scan5<false, true>; break;
    case KERNEL_SCAN5_WIDE: kernel = k_scan5<true, true>; break;
    case KERNEL_SCAN4S: kernel = k_scan4s<true>; break;
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(SCAN_BLOCK), 0, stream, args);
}

void launch_assign7_ordered(int grid, hipStream_t stream, const Hit7* hits,
                            unsigned long long nhits, DevCtl* ctl, u64 seed) {
  hipLaunchKernelGGL(k_scan7_assign<true>, dim3(grid), dim3(SCAN_BLOCK), 0,
                     stream, hits, nhits, ctl, seed);
}

}  // namespace sbg
