// scan4s.hpp — the shared-input two-LUT scan kernel k_scan4s and its
// survivor routine. Included by the kernel modules only (scan_launch.hpp).
#pragma once

#include "scan_device.hpp"

namespace sbg {
namespace {

// ---------------------------------------------------------------------------
// K3s — shared-input two-LUT scan over 4-combinations: LUT(LUT(x,y,z), d, s)
// with s one of x, y, z (lut4s_solve_from_p). Workgroups dequeue batches of
// SB triple prefixes (a,b,c), the prefix-batch layer of k_scan5; a prefix's
// row is short (its tail gates d in (c, n)), so a batch packs SB of them to
// keep the waves full. One thread per (prefix, d): it splits the live
// prefix cells by its own table, and a cell forced both ways ends the
// candidate; what is left goes to the 12-shape solver.
// ---------------------------------------------------------------------------

// Survivor handling for k_scan4s (noinline, as scan5_handle_survivor): exact
// 16-cell p-masks, then the solver.
template <bool ORD>
__device__ __attribute__((noinline)) void scan4s_handle_survivor(
    const ScanArgs& args, DevCtl* ctl, const u64* s_pool, const u16* abc,
    i64 rank, int d) {
  ttable tt4[4];
  const u16 nums[4] = {abc[0], abc[1], abc[2], static_cast<u16>(d)};
  for (int j = 0; j < 4; j++) {
    for (int w = 0; w < 4; w++) tt4[j].w[w] = s_pool[nums[j] * PSTR + w];
  }
  u32 p1, p0;
  if (!lut4_p_masks(tt4, args.T1, args.T0, &p1, &p0)) return;
  u8 fo, fi;
  int shape;
  if (!lut4s_solve_from_p(p1, p0, scan_rnd(args.seed, rank), &fo, &fi, &shape)) {
    return;
  }
  if (args.count_all) return;
  if constexpr (ORD) {
    dev_lower_best(ctl, static_cast<u64>(rank));
    return;
  }
  u8 pos[5];
  lut4s_shape_gates(shape, pos);
  u16 res[10] = {};
  res[0] = fo;
  res[1] = fi;
  for (int j = 0; j < 5; j++) res[2 + j] = nums[pos[j]];
  dev_publish(ctl, res);
}

template <bool ORD>
__global__ void __launch_bounds__(SCAN_BLOCK, 4) k_scan4s(ScanArgs args) {
  __shared__ alignas(16) u64 s_pool[MAX_GATES * PSTR];
  __shared__ alignas(16) u64 s_H1[SB][8][4];
  __shared__ alignas(16) u64 s_H0[SB][8][4];
  __shared__ i64 s_base[SB];       // flat-rank base of each prefix
  __shared__ i64 s_prefix[SB + 1]; // prefix sums of the window sizes
  __shared__ int s_lo[SB];         // window start (tail index) per prefix
  __shared__ u16 s_abc[SB][3];
  __shared__ u32 s_live[SB];       // cells with both forced-1 and forced-0
                                   // content; only these can contradict
  __shared__ i64 s_batch;          // first triple index of the batch
  __shared__ int s_stop;           // all prefixes past range end

  const int n = args.n;
  load_pool_lds(s_pool, args.pool, n);  // published by the first dequeue

  DevCtl* ctl = args.ctl;
  const i64 total3 = cf3(n);
  u64 local_eval = 0;

  for (;;) {
    const i64 batch_base =
        dequeue_batch<ORD>(ctl, SB, args.count_all, false, &s_batch);
    if (batch_base < 0) break;

    if (threadIdx.x < SB) {
      const int t = threadIdx.x;
      PrefixWindow<3> p =
          decode_prefix_window<3, 4>(batch_base + t, total3, args);
      drop_dead_prefix(p, args);
      s_base[t] = p.base;
      s_lo[t] = static_cast<int>(p.lo);  // < m <= MAX_GATES
      for (int j = 0; j < 3; j++) s_abc[t][j] = static_cast<u16>(p.ids[j]);
      s_prefix[t + 1] = p.hi - p.lo;  // count, turned into prefix sums below
      if (t == 0) s_prefix[0] = 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      // Termination as in k_scan5: flat-rank bases increase with the triple
      // index, so once the batch's first triple is past the range end (or
      // past the triple space), every later batch is too.
      s_stop = (batch_base >= total3 || s_base[0] >= args.end) ? 1 : 0;
      if constexpr (ORD) {  // as in k_scan5
        if (!s_stop && static_cast<u64>(s_base[0]) > dev_best(ctl)) s_stop = 1;
      }
      for (int t = 0; t < SB; t++) s_prefix[t + 1] += s_prefix[t];
    }
    __syncthreads();
    if (s_stop) break;
    const int total_cands = static_cast<int>(s_prefix[SB]);  // <= SB * n
    if (total_cands == 0) continue;

    build_prefix_cells<3, SB>(s_pool, s_abc, s_prefix, args.T1, args.T0, s_H1,
                              s_H0);
    static_assert(SB * 8 <= SCAN_BLOCK);  // mark_live_cells: a thread a cell
    mark_live_cells<3, SB>(s_H1, s_H0, s_live);
    __syncthreads();

    int it = 0;
    for (int idx = threadIdx.x; idx < total_cands; idx += blockDim.x) {
      // Ordered: a batch that was begun runs to its end, as in k_scan5.
      if (!ORD && ((it++) & 15) == 0 && !args.count_all && dev_abort(ctl)) {
        break;
      }
      // The prefix of candidate idx: the last t with s_prefix[t] <= idx.
      int t = 0;
#pragma unroll
      for (int step = SB / 2; step > 0; step >>= 1) {
        if (s_prefix[t + step] <= idx) t += step;
      }
      const int q = s_lo[t] + (idx - static_cast<int>(s_prefix[t]));
      const int d = s_abc[t][2] + 1 + q;
      if (args.excl != 0 && dev_excluded(args.excl, d)) continue;
      local_eval++;

      u64 td_[4];
#pragma unroll
      for (int w = 0; w < 4; w++) td_[w] = s_pool[d * PSTR + w];
      bool ok = true;
      for (u32 lm = s_live[t]; lm != 0 && ok; lm &= lm - 1) {
        const int u = __ffs(lm) - 1;
        u64 a1 = 0, n1 = 0, a0 = 0, n0 = 0;
#pragma unroll
        for (int w = 0; w < 4; w++) {
          const u64 h1 = s_H1[t][u][w];
          const u64 h0 = s_H0[t][u][w];
          const u64 x1 = h1 & td_[w];
          const u64 x0 = h0 & td_[w];
          a1 |= x1;
          n1 |= h1 ^ x1;
          a0 |= x0;
          n0 |= h0 ^ x0;
        }
        if ((a1 != 0 && a0 != 0) || (n1 != 0 && n0 != 0)) ok = false;
      }
      if (!ok) continue;
      scan4s_handle_survivor<ORD>(args, ctl, s_pool, s_abc[t], s_base[t] + q,
                                  d);
    }
  }

  block_add_evaluated(ctl, local_eval);
}

}  // namespace
}  // namespace sbg
