// scan_pairs.hpp — the one-shot pair scan kernel k_scan2. It has one variant
// (the pair scan reports its lowest hit as it is), and a kernel that is not
// a template is emitted by every module that sees it, so this header is
// included by scan_default.hip alone.
#pragma once

#include "scan_device.hpp"

namespace sbg {
namespace {

// K1p — gate-mode step-3/4a pair scan, one-shot launch: one thread per pair
// rank, grid-stride, the launch shape of k_scan3. The lowest hit rank lands
// in ctl->best (walk_pairs in scan_device.hpp); the host derives the result.
__global__ void __launch_bounds__(SCAN_BLOCK) k_scan2(ScanArgs args) {
  __shared__ alignas(16) u64 s_pool[MAX_GATES * PSTR];
  __shared__ alignas(16) Pair2Stage s_pair2;
  load_pool_lds(s_pool, args.pool, args.n);
  copy_pair2_stage(&s_pair2, args.pair2);
  __syncthreads();

  const i64 stride = static_cast<i64>(gridDim.x) * blockDim.x;
  const i64 idx0 =
      args.begin + blockIdx.x * static_cast<i64>(blockDim.x) + threadIdx.x;
  walk_pairs(s_pool, &s_pair2, args.n, args.T1, args.T0, args.ctl, idx0,
             args.end, stride);
}

}  // namespace
}  // namespace sbg
