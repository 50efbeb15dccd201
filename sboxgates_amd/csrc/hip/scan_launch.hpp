// scan_launch.hpp — typed launchers of the one-shot scan kernels for CDNA4
// (gfx950): the 3/5/7-LUT, shared-input two-LUT, k=4 triple and k=2 pair
// candidate scans. Host wrapper: gpu_engine.hip; persistent k=4 / k=2
// service: scan_service.hip. Private to csrc/hip.
//
// Design (MI355X-first; see SURVEY.md §2.3 and the repo README):
//  * One thread evaluates one candidate combination on 256-bit truth
//    tables held as 4 u64 words. The reference runs these scans as CPU
//    loops across MPI ranks (lut.c:116-487); here the per-candidate
//    feasibility test is restructured as incremental cell algebra
//    (sbg/lutcover.hpp) with a per-u early exit.
//  * The live gate pool (<= 500 x 32 B = 16 KB) is staged in LDS once per
//    workgroup; the shared outer-prefix cells (8 for 5-LUT, 16 for 7-LUT)
//    are computed once per prefix and broadcast-read from LDS, so the
//    inner loop touches only the candidate's own 2-3 tables.
//  * Work distribution: workgroups pull combination *prefixes* (triples
//    for K5, quadruples for K7) from a device-scope atomic queue — the
//    per-prefix work varies by orders of magnitude, and the dequeue
//    primitive costs ~0.25-1 us (MI355X_MICROARch price list), negligible
//    against per-prefix work. Grids are sized >> 256 CUs.
//  * Early exit: winner election by atomicCAS on a device-scope lock; an
//    agent-scope abort flag (sc1, L1-bypassing load) is polled on a coarse
//    cadence. By default any valid winner is acceptable (the reference is
//    equally nondeterministic across ranks, lut.c:213-218).
//  * Ordered scans (ScanRequest::ordered): the winner is the hit of the
//    lowest rank, which is what the CPU scan of the same window returns. A
//    hit only lowers ctl->best with one fetch_min (dev_lower_best), as the
//    pair scan does; no lock, no payload, no abort flag, no waiting. best
//    is read to skip work that ranks above it: the strided walks leave
//    once past it, the prefix queue stops handing out batches, and a batch
//    already taken that begins below it runs to its end. The host reads
//    the rank back and derives the result words with the CPU scan of that
//    single rank. Every kernel that differs takes the mode as a template
//    parameter.
//
// Files: the kernels are templates in one header per family
// (scan_strided.hpp, scan_pairs.hpp, scan5.hpp, scan4s.hpp,
// scan7_filter.hpp, scan7_assign.hpp) over the shared device code of
// scan_device.hpp, and two modules instantiate them: scan_default.hip the
// default mode and the kernels that have one variant (k_scan2,
// k_scan7_filter), scan_ordered.hip the ordered mode. Two modules, because
// the default kernels then compile to exactly the code they had before there
// was a second mode: with both instantiations in one module the optimizer
// scheduled the default k_scan5 differently (same registers, same scratch,
// 0.4% slower on the 5-LUT benchmark; profiles/ordered_scans.md §1). For the
// same reason k_scan5_wave, in both modes, is a third module, scan_wave.hip:
// with it in the other two, k_scan5 and scan5_wide_walk came out different
// (they share the survivor routine with it). No kernel is named outside
// those three modules.
#pragma once

#include <hip/hip_runtime.h>

#include "scan_types.hpp"

namespace sbg {

enum ScanKernel {
  KERNEL_SCAN2,          // one variant
  KERNEL_SCAN3,
  KERNEL_SCAN4,
  KERNEL_SCAN5_ROWS,     // k_scan5<false, ...>: pools without a long row
  KERNEL_SCAN5_WIDE,     // k_scan5<true, ...>
  KERNEL_SCAN4S,
  KERNEL_SCAN7_FILTER,   // one variant
};

// Launch `which` on `grid` workgroups of SCAN_BLOCK threads, one function
// per module. launch_scan_ordered hands a kernel that has one variant on to
// launch_scan_default.
void launch_scan_default(ScanKernel which, int grid, hipStream_t stream,
                         const ScanArgs& args);
void launch_scan_ordered(ScanKernel which, int grid, hipStream_t stream,
                         const ScanArgs& args);

// Launch k_scan5_wave on the queue of q_units triples from q_begin on.
void launch_scan5_wave_default(int grid, hipStream_t stream,
                               const ScanArgs& args, i64 q_begin, i64 q_units);
void launch_scan5_wave_ordered(int grid, hipStream_t stream,
                               const ScanArgs& args, i64 q_begin, i64 q_units);

// Launch k_scan7_assign over nhits entries of the buffer `hits`; ctl is the
// device control block, whose pool_n holds the pool size in the ordered mode.
void launch_assign7_default(int grid, hipStream_t stream, const Hit7* hits,
                            unsigned long long nhits, DevCtl* ctl, u64 seed);
void launch_assign7_ordered(int grid, hipStream_t stream, const Hit7* hits,
                            unsigned long long nhits, DevCtl* ctl, u64 seed);

// The kernel in the mode of the scan.
inline void launch_scan(ScanKernel which, bool ordered, int grid,
                        hipStream_t stream, const ScanArgs& args) {
  (ordered ? launch_scan_ordered : launch_scan_default)(which, grid, stream,
                                                        args);
}
inline void launch_scan5_wave(bool ordered, int grid, hipStream_t stream,
                              const ScanArgs& args, i64 q_begin,
                              i64 q_units) {
  (ordered ? launch_scan5_wave_ordered : launch_scan5_wave_default)(
      grid, stream, args, q_begin, q_units);
}
inline void launch_assign7(bool ordered, int grid, hipStream_t stream,
                           const Hit7* hits, unsigned long long nhits,
                           DevCtl* ctl, u64 seed) {
  (ordered ? launch_assign7_ordered : launch_assign7_default)(
      grid, stream, hits, nhits, ctl, seed);
}

}  // namespace sbg
