// scan_strided.hpp — the one-shot kernels that walk triple ranks with a grid
// stride: k_scan3 (3-LUT scan) and k_scan4 (gate-mode step-4 triple scan).
// Included by the kernel modules only (scan_launch.hpp).
//
// ORD, here and on the kernels of the other families: the ordered variant
// (see "Ordered scans" in scan_launch.hpp), a compile-time parameter so that
// the default kernels are what they were without it. scan_default.hip
// instantiates ORD = false only and scan_ordered.hip ORD = true only.
#pragma once

#include "scan_device.hpp"

namespace sbg {
namespace {

// ---------------------------------------------------------------------------
// K2 — 3-LUT scan. Grid-stride over combination ranks; per-thread decode by
// binary search on closed-form binomials; cells evaluated directly (the
// reference's serial rank-0 loop, lut.c:501-523).
// ---------------------------------------------------------------------------
template <bool ORD>
__global__ void __launch_bounds__(SCAN_BLOCK) k_scan3(ScanArgs args) {
  __shared__ alignas(16) u64 s_pool[MAX_GATES * PSTR];
  load_pool_lds(s_pool, args.pool, args.n);
  __syncthreads();

  DevCtl* ctl = args.ctl;
  const i64 stride = static_cast<i64>(gridDim.x) * blockDim.x;
  const i64 idx0 =
      args.begin + blockIdx.x * static_cast<i64>(blockDim.x) + threadIdx.x;
  const u64 local_eval = walk_triples<ORD>(
      s_pool, args.n, args.T1, args.T0, args.count_all, ctl, idx0, args.end,
      stride, [&](i64 idx, int a, int b, int c, u32 p1, u32 p0) {
        // Same random word as cpu_scan3 (see scan_rnd in sbg/rng.hpp).
        u8 func = lut3_function_from_p(
            p1, p0, hash_mix64(args.seed ^ static_cast<u64>(idx)));
        if (args.count_all || func == 0) return false;
        if constexpr (ORD) {
          dev_lower_best(ctl, static_cast<u64>(idx) << BEST3_SHIFT);
          return true;
        }
        u16 res[10] = {};
        res[0] = func;
        res[1] = static_cast<u16>(a);
        res[2] = static_cast<u16>(b);
        res[3] = static_cast<u16>(c);
        dev_publish(ctl, res);
        return true;
      });
  block_add_evaluated(ctl, local_eval);
}

// K1c — gate-mode step-4 triple scan, one-shot launch (Scan4Match in
// scan_device.hpp is the per-triple function search).
template <bool ORD>
__global__ void __launch_bounds__(SCAN_BLOCK) k_scan4(ScanArgs args) {
  __shared__ alignas(16) u64 s_pool[MAX_GATES * PSTR];
  __shared__ alignas(16) u8 s_bitmap[MATCHER_BITMAP_BYTES];
  __shared__ u8 s_funs[256];
  __shared__ int s_count;
  load_pool_lds(s_pool, args.pool, args.n);
  load_matcher_lds(s_bitmap, s_funs, &s_count, args.matcher);
  __syncthreads();

  DevCtl* ctl = args.ctl;
  const i64 stride = static_cast<i64>(gridDim.x) * blockDim.x;
  const i64 idx0 =
      args.begin + blockIdx.x * static_cast<i64>(blockDim.x) + threadIdx.x;
  const u64 local_eval = walk_triples<ORD>(
      s_pool, args.n, args.T1, args.T0, args.count_all, ctl, idx0, args.end,
      stride, Scan4Match<ORD>{s_bitmap, s_funs, s_count, args.count_all, ctl});
  block_add_evaluated(ctl, local_eval);
}

}  // namespace
}  // namespace sbg
