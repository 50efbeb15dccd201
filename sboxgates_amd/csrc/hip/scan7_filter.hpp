// scan7_filter.hpp — first half of the 7-LUT scan: the feasibility filter
// k_scan7_filter and its survivor routine. The filter has one variant (no
// hit ever aborts it), and a kernel that is not a template is emitted by
// every module that sees it, so this header is included by scan_default.hip
// alone. Second half: scan7_assign.hpp.
#pragma once

#include "scan_device.hpp"

namespace sbg {
namespace {

// ---------------------------------------------------------------------------
// K4a — 7-LUT feasibility filter. Workgroups dequeue quadruple prefixes;
// 16 prefix cells in LDS; threads screen (e, f, g) triples; survivors'
// p-masks land in the hit buffer (no 100k cap — 288 GB HBM keeps the whole
// frontier resident; overflow of the per-chunk buffer is reported and the
// host re-scans a smaller range).
// ---------------------------------------------------------------------------
// Survivor handling for k_scan7_filter: exact p-mask rebuild + hit append.
__device__ __attribute__((noinline)) void scan7_handle_survivor(
    const ScanArgs& args, DevCtl* ctl, const u64* s_pool, const u16* abcd,
    int e, int f, int g) {
  ttable tt7[7];
  const int ids[7] = {abcd[0], abcd[1], abcd[2], abcd[3], e, f, g};
  for (int j = 0; j < 7; j++) {
    for (int w = 0; w < 4; w++) tt7[j].w[w] = s_pool[ids[j] * PSTR + w];
  }
  u64 p1[2], p0[2];
  if (!lut7_p_masks(tt7, args.T1, args.T0, p1, p0)) return;
  if (args.count_all) return;  // bench mode: no hit materialization
  unsigned long long slot = __hip_atomic_fetch_add(&ctl->hit_count, 1ULL,
                                                   __ATOMIC_RELAXED,
                                                   __HIP_MEMORY_SCOPE_AGENT);
  if (slot >= args.hit_cap) {
    __hip_atomic_store(&ctl->overflow, 1u, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  Hit7& h = args.hits[slot];
  h.p1[0] = p1[0];
  h.p1[1] = p1[1];
  h.p0[0] = p0[0];
  h.p0[1] = p0[1];
  for (int j = 0; j < 7; j++) h.nums[j] = static_cast<u16>(ids[j]);
}

__global__ void __launch_bounds__(SCAN_BLOCK, 4) k_scan7_filter(ScanArgs args) {
  // Quad batching: one dequeue + one cooperative 16-cell build per QB
  // quadruples (same barrier-amortization pattern as k_scan5).
  __shared__ alignas(16) u64 s_pool[MAX_GATES * PSTR];
  __shared__ alignas(16) u64 s_H1[QB][16][4];
  __shared__ alignas(16) u64 s_H0[QB][16][4];
  __shared__ i64 s_lo[QB], s_prefix[QB + 1];
  __shared__ int s_m[QB], s_d[QB];
  __shared__ u16 s_abcd[QB][4];
  __shared__ u32 s_live[QB];
  __shared__ i64 s_batch;  // first unit (quad x slice) index of the batch
  __shared__ i64 s_first;  // flat-rank base of the batch's first quad
  __shared__ int s_stop;

  const int n = args.n;
  load_pool_lds(s_pool, args.pool, n);

  DevCtl* ctl = args.ctl;
  const i64 total4 = cf4(n);
  u64 local_eval = 0;

  for (;;) {
    const i64 batch_base =
        dequeue_batch(ctl, QB, args.count_all, true, &s_batch);
    if (batch_base < 0) break;

    if (threadIdx.x < QB) {
      const int t = threadIdx.x;
      const int S = args.slices7;
      const i64 unit = batch_base + t;
      const i64 qidx = unit / S;
      const int slice = static_cast<int>(unit % S);
      PrefixWindow<4> p = decode_prefix_window<4>(qidx, total4, args);
      if (S > 1 && p.hi > p.lo) {
        // This unit covers one slice of the quad's triple window.
        const i64 span = p.hi - p.lo;
        const i64 per = (span + S - 1) / S;
        const i64 s_lo2 = p.lo + per * slice;
        const i64 s_hi2 = s_lo2 + per < p.hi ? s_lo2 + per : p.hi;
        p.lo = s_lo2 < p.hi ? s_lo2 : p.hi;
        p.hi = s_hi2;
      }
      drop_dead_prefix(p, args);
      if (t == 0) {
        s_first = p.base;
        s_prefix[0] = 0;
      }
      s_lo[t] = p.lo;
      s_m[t] = p.m;
      s_d[t] = p.ids[3];
      for (int j = 0; j < 4; j++) s_abcd[t][j] = static_cast<u16>(p.ids[j]);
      s_prefix[t + 1] = p.hi - p.lo;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      s_stop = (batch_base / args.slices7 >= total4 || s_first >= args.end)
                   ? 1
                   : 0;
      for (int t = 0; t < QB; t++) s_prefix[t + 1] += s_prefix[t];
    }
    __syncthreads();
    if (s_stop) break;
    const i64 total_trips = s_prefix[QB];
    if (total_trips == 0) continue;

    build_prefix_cells<4, QB>(s_pool, s_abcd, s_prefix, args.T1, args.T0, s_H1,
                              s_H0);
    mark_live_cells<4, QB>(s_H1, s_H0, s_live);
    __syncthreads();

    int it = 0;
    for (i64 idx = threadIdx.x; idx < total_trips; idx += blockDim.x) {
      if (((it++) & 15) == 0) {
        if ((!args.count_all && dev_abort(ctl)) ||
            __hip_atomic_load(&ctl->overflow, __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT) != 0) {
          break;
        }
      }
      int t = 0;
      while (s_prefix[t + 1] <= idx) t++;
      const i64 q = s_lo[t] + (idx - s_prefix[t]);
      const int m = s_m[t];
      const int dgate = s_d[t];
      int e2, f2, g2;
      dev_decode_triple(q, m, &e2, &f2, &g2);
      int e = dgate + 1 + e2, f = dgate + 1 + f2, g = dgate + 1 + g2;
      if (args.excl != 0) {
        if (dev_excluded(args.excl, e) || dev_excluded(args.excl, f) ||
            dev_excluded(args.excl, g)) {
          continue;
        }
      }
      local_eval++;

      u64 te_[4], tf_[4], tg_[4];
#pragma unroll
      for (int w = 0; w < 4; w++) {
        te_[w] = s_pool[e * PSTR + w];
        tf_[w] = s_pool[f * PSTR + w];
        tg_[w] = s_pool[g * PSTR + w];
      }

      bool ok = true;
      for (u32 lm = s_live[t]; lm != 0 && ok; lm &= lm - 1) {
        const int u = __ffs(lm) - 1;
        u64 acc1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        u64 acc0[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int w = 0; w < 4; w++) {
          const u64 h1 = s_H1[t][u][w];
          const u64 h0 = s_H0[t][u][w];
          const u64 e1 = h1 & te_[w];
          const u64 e0n = h1 ^ e1;
          const u64 z1 = h0 & te_[w];
          const u64 z0n = h0 ^ z1;
          const u64 ef11 = e1 & tf_[w];
          const u64 ef10 = e1 ^ ef11;
          const u64 ef01 = e0n & tf_[w];
          const u64 ef00 = e0n ^ ef01;
          const u64 zf11 = z1 & tf_[w];
          const u64 zf10 = z1 ^ zf11;
          const u64 zf01 = z0n & tf_[w];
          const u64 zf00 = z0n ^ zf01;
          u64 x;
          x = ef11 & tg_[w]; acc1[7] |= x; acc1[6] |= ef11 ^ x;
          x = ef10 & tg_[w]; acc1[5] |= x; acc1[4] |= ef10 ^ x;
          x = ef01 & tg_[w]; acc1[3] |= x; acc1[2] |= ef01 ^ x;
          x = ef00 & tg_[w]; acc1[1] |= x; acc1[0] |= ef00 ^ x;
          x = zf11 & tg_[w]; acc0[7] |= x; acc0[6] |= zf11 ^ x;
          x = zf10 & tg_[w]; acc0[5] |= x; acc0[4] |= zf10 ^ x;
          x = zf01 & tg_[w]; acc0[3] |= x; acc0[2] |= zf01 ^ x;
          x = zf00 & tg_[w]; acc0[1] |= x; acc0[0] |= zf00 ^ x;
        }
#pragma unroll
        for (int pp = 0; pp < 8; pp++) {
          if (acc1[pp] && acc0[pp]) {
            ok = false;
            break;
          }
        }
      }
      if (!ok) continue;
      scan7_handle_survivor(args, ctl, s_pool, s_abcd[t], e, f, g);
    }
  }

  block_add_evaluated(ctl, local_eval);
}

}  // namespace
}  // namespace sbg
