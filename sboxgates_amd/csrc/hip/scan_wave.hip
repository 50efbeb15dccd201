// scan_wave.hip — the module of k_scan5_wave, the wide 5-LUT kernel whose
// waves own their triples, in both modes, with its launchers. A module of
// its own, so that scan_default.hip and scan_ordered.hip compile to exactly
// the code they had without it (why that matters: scan_launch.hpp).

#include "scan_launch.hpp"
#include "scan5.hpp"

namespace sbg {

void launch_scan5_wave_default(int grid, hipStream_t stream,
                               const ScanArgs& args, i64 q_begin,
                               i64 q_units) {
  hipLaunchKernelGGL(k_scan5_wave<false>, dim3(grid), dim3(SCAN_BLOCK), 0,
                     stream, args, q_begin, q_units);
}

void launch_scan5_wave_ordered(int grid, hipStream_t stream,
                               const ScanArgs& args, i64 q_begin,
                               i64 q_units) {
  hipLaunchKernelGGL(k_scan5_wave<true>, dim3(grid), dim3(SCAN_BLOCK), 0,
                     stream, args, q_begin, q_units);
}

}  // namespace sbg
