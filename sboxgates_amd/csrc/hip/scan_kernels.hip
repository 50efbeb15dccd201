// scan_kernels.hip — CDNA4 (gfx950) one-shot kernels for the 3/5/7-LUT,
// shared-input two-LUT and k=4 candidate scans, plus the GpuEngine host wrapper. Shared device code:
// scan_device.hpp; persistent k=4 service: scan_service.hip.
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

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>

#include "sbg/comb.hpp"
#include "sbg/scan5_geom.hpp"
#include "scan_device.hpp"
#include "scan_ordered.hpp"
#include "scan_service.hpp"

namespace sbg {

namespace {

// Batch sizes and split factors, shared by the kernels and the host code
// that sizes their grids.
constexpr int TB = 8;        // k_scan5: triple prefixes per dequeue
constexpr int SB = 16;       // k_scan4s: triple prefixes per dequeue (a power
                             // of two: the candidate's prefix is found by
                             // binary search)
constexpr int QB = 4;        // k_scan7_filter: quad units per dequeue
constexpr u64 FM_SPLIT = 8;  // k_scan7_assign: threads per (hit, ordering)
// k_scan7_filter: candidates one dequeue unit should hold; the host slices
// quads until a scan has about one unit per this many candidates.
constexpr i64 SLICE_UNIT = 8 * SCAN_BLOCK;

// ---------------------------------------------------------------------------
// K2 — 3-LUT scan. Grid-stride over combination ranks; per-thread decode by
// binary search on closed-form binomials; cells evaluated directly (the
// reference's serial rank-0 loop, lut.c:501-523).
//
// ORD, here and on the kernels below: the ordered variant (see the Early
// exit note above), a compile-time parameter so that the default kernels
// are what they were without it. This file instantiates ORD = false only;
// scan_ordered.hip includes it with SBG_ORDERED_TU defined and instantiates
// ORD = true, behind the launchers at the end (why: scan_ordered.hpp).
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

#ifndef SBG_ORDERED_TU  // the pair scan has one variant
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
#endif  // SBG_ORDERED_TU

// ---------------------------------------------------------------------------
// K3 — 5-LUT scan. Workgroups dequeue triple prefixes; the 8 prefix cells
// (masked with target-1/target-0) are computed cooperatively into LDS; each
// thread then takes one row d and a run of e's, screens the e's against
// the most balanced live cell, sends what passes through the remaining
// live cells, and runs the 2-coloring decomposition solver on survivors
// (replacing the reference's 10 x 256-function brute force,
// lut.c:174-246). Short rows: 4 consecutive e per task, d side hoisted
// into registers, e's tables read row by row. Long rows: 64 e per task,
// taken a table position at a time from the gate-transposed pool.
// ---------------------------------------------------------------------------

// Survivor handling for k_scan5 (rare path; noinline keeps its registers
// out of the hot loop's budget). STR: the pool's LDS stride. ORD: a hit
// lowers ctl->best with its rank; the host derives the result words.
template <int STR, bool ORD>
__device__ __attribute__((noinline)) void scan5_handle_survivor(
    const ScanArgs& args, DevCtl* ctl, const u64* s_pool, const u16* abc,
    i64 rank, int d, int e) {
  ttable tt5[5];
  const int ids[5] = {abc[0], abc[1], abc[2], d, e};
  for (int j = 0; j < 5; j++) {
    for (int w = 0; w < 4; w++) tt5[j].w[w] = s_pool[ids[j] * STR + w];
  }
  u32 p1, p0;
  if (!lut5_p_masks(tt5, args.T1, args.T0, &p1, &p0)) return;
  u8 fo, fi;
  int split;
  if (!lut5_solve_from_p(p1, p0, scan_rnd(args.seed, rank), &fo, &fi, &split)) {
    return;
  }
  if (args.count_all) return;
  if constexpr (ORD) {
    dev_lower_best(ctl, static_cast<u64>(rank));
    return;
  }
  const u16 nums[5] = {abc[0], abc[1], abc[2], static_cast<u16>(d),
                       static_cast<u16>(e)};
  const u8* sp = SPLITS5[split];
  u16 res[10] = {};
  res[0] = fo;
  res[1] = fi;
  for (int j = 0; j < 3; j++) res[2 + j] = nums[sp[j]];
  res[5] = nums[sp[3]];
  res[6] = nums[sp[4]];
  dev_publish(ctl, res);
}

// The same test as the screen's on the remaining live cells of pair (d, e),
// then the solver. Shared by both walks of k_scan5.
template <int STR, bool ORD>
__device__ __forceinline__ void scan5_after_screen(
    const ScanArgs& args, DevCtl* ctl, const u64* s_pool,
    const u64 (*H1)[4], const u64 (*H0)[4], const u16* abc, u32 other_live,
    i64 rank, int d, int e) {
  u64 td_[4], te_[4];
#pragma unroll
  for (int w = 0; w < 4; w++) {
    td_[w] = s_pool[d * STR + w];
    te_[w] = s_pool[e * STR + w];
  }
  for (u32 lm = other_live; lm != 0; lm &= lm - 1) {
    const int u = __ffs(lm) - 1;
    u64 r11_1 = 0, r10_1 = 0, r01_1 = 0, r00_1 = 0;
    u64 r11_0 = 0, r10_0 = 0, r01_0 = 0, r00_0 = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      const u64 h1 = H1[u][w];
      const u64 h0 = H0[u][w];
      // x & ~y == x ^ (x & y): avoids materializing ~td/~te.
      const u64 a1 = h1 & td_[w];
      const u64 na1 = h1 ^ a1;
      const u64 a0 = h0 & td_[w];
      const u64 na0 = h0 ^ a0;
      const u64 x11_1 = a1 & te_[w];
      const u64 x01_1 = na1 & te_[w];
      const u64 x11_0 = a0 & te_[w];
      const u64 x01_0 = na0 & te_[w];
      r11_1 |= x11_1;
      r10_1 |= a1 ^ x11_1;
      r01_1 |= x01_1;
      r00_1 |= na1 ^ x01_1;
      r11_0 |= x11_0;
      r10_0 |= a0 ^ x11_0;
      r01_0 |= x01_0;
      r00_0 |= na0 ^ x01_0;
    }
    if ((r11_1 && r11_0) || (r10_1 && r10_0) || (r01_1 && r01_0) ||
        (r00_1 && r00_0)) {
      return;
    }
  }
  scan5_handle_survivor<STR, ORD>(args, ctl, s_pool, abc, rank, d, e);
}

// LDS pointers, for k_scan5's arrays as arguments of its wide walk (a plain
// pointer argument would turn every read into a flat access).
typedef __attribute__((address_space(3))) const u64 lds_cu64;
typedef __attribute__((address_space(3))) const u32 lds_cu32;
typedef __attribute__((address_space(3))) const u16 lds_cu16;
typedef __attribute__((address_space(3))) const u8 lds_cu8;

// Wide walk of one batch of k_scan5<true>: returns the pairs this thread
// evaluated. Consecutive lanes take consecutive rows d of one word group,
// last group first (it has the most rows, so the per-lane search for the
// group is short). A wave holds one triple and mostly one group: its lanes
// read the same G dwords (LDS broadcast), and each brings its own td. Not
// inlined: the kernel's other walk needs most of the register file, and
// inside the kernel this loop's invariants were spilled and reloaded from
// scratch in every task; as a function it gets registers of its own.
template <int STR, bool ORD>
__device__ __attribute__((noinline)) u64 scan5_wide_walk(
    const ScanArgs& args, DevCtl* ctl, int pad, int total_tasks,
    lds_cu64* l_pool, lds_cu32* l_G, lds_cu32* l_tpre, lds_cu32* l_rec,
    lds_cu8* l_pos, lds_cu64* l_H1, lds_cu64* l_H0, lds_cu16* l_abc,
    lds_cu64* l_base) {
  constexpr int NW = SCAN5_WIDE_WORDS;
  constexpr int GB = SCAN5_WIDE_GB;
  const u64* s_pool = (const u64*)l_pool;
  const u32* s_G = (const u32*)l_G;
  const u32* s_tpre = (const u32*)l_tpre;                      // [TB + 1]
  const u32 (*s_rec)[16] = (const u32 (*)[16])l_rec;          // [TB]
  const u8 (*s_pos)[GT_LIST_BYTES] = (const u8 (*)[GT_LIST_BYTES])l_pos;
  const u64 (*s_H1)[8][4] = (const u64 (*)[8][4])l_H1;        // [TB]
  const u64 (*s_H0)[8][4] = (const u64 (*)[8][4])l_H0;
  const u16 (*s_abc)[3] = (const u16 (*)[3])l_abc;            // [TB]
  const i64* s_base = (const i64*)l_base;                      // [TB]
  const int n = args.n;
  const int count_all = args.count_all;
  const u64 excl = args.excl;
  u64 local_eval = 0;
  int since_poll = 0;
  for (int task = threadIdx.x; task < total_tasks; task += blockDim.x) {
    if (!count_all) {
      since_poll += GB;
      if (since_poll >= 64) {
        since_poll = 0;
        // An ordered scan runs a batch it has begun to its end: the batch
        // lies below the best hit known when it was taken.
        if (!ORD && dev_abort(ctl)) break;
      }
    }
    // Task counts are padded to the wave size, so a wave holds one
    // triple: the one of its first task, found by 8 lanes at once.
    const int task0 = __builtin_amdgcn_readfirstlane(task);
    const u64 below = __ballot(
        static_cast<int>(s_tpre[1 + (threadIdx.x & 7)]) <= task0);
    const int t = __popc(static_cast<u32>(below) & ((1u << TB) - 1u));
    // The triple's record, through scalars.
    const lds_u32x4* rec = reinterpret_cast<const lds_u32x4*>(s_rec[t]);
    const lds_u32x4 ra = rec[0], rh1 = rec[2], rh0 = rec[3];
    const lds_u32x2 rb = *reinterpret_cast<const lds_u32x2*>(&s_rec[t][4]);
    const int tpre = __builtin_amdgcn_readfirstlane(ra.x);
    const int cnt = __builtin_amdgcn_readfirstlane(ra.y);
    const int lo = __builtin_amdgcn_readfirstlane(ra.z);
    const int hi = __builtin_amdgcn_readfirstlane(ra.w);
    const u32 ids = dev_uniform(rb.x);
    const u32 lens = dev_uniform(rb.y);
    const u32 head1[4] = {dev_uniform(rh1.x), dev_uniform(rh1.y),
                          dev_uniform(rh1.z), dev_uniform(rh1.w)};
    const u32 head0[4] = {dev_uniform(rh0.x), dev_uniform(rh0.y),
                          dev_uniform(rh0.z), dev_uniform(rh0.w)};
    const int task_t = task - tpre;
    if (task_t >= cnt) continue;
    // Bit i of the task is the pair (d, e0 + i), flat index q0 + i;
    // valid: clipped to e > d and to the triple's [lo, hi) window,
    // without the excluded gates.
    const Scan5WideTask wt =
        scan5_wide_decode(n, pad, static_cast<int>(ids & 0xffffu), task_t);
    const int wg = wt.wg, d = wt.d, e0 = wt.e0, q0 = wt.q0;
    const u64 valid = scan5_wide_valid(wt, lo, hi, excl);
    if (valid == 0) continue;
    local_eval += __popcll(valid);

    // Screen: the listed positions of the screen cell. Per position the
    // lanes read G at their candidate words (the same address across most
    // of a wave: LDS broadcast) and at d's own word for td's bit. A cell
    // that is not live has one side empty and rejects nothing, as in the
    // short walk.
    const u32 live = (ids >> 16) & 0xffu;
    const int u0 = static_cast<int>(ids >> 24);
    const int n1 = static_cast<int>(lens & 0x3ffu);
    const int n0 = static_cast<int>((lens >> 10) & 0x3ffu);
    GtWords<NW> vw;
#pragma unroll
    for (int k = 0; k < NW; k++) {
      vw.w[k] = static_cast<u32>(valid >> (32 * k));
    }
    const GtWords<NW> pw = gt_screen<NW>(
        head1, head0, s_pos[t], n1, s_pos[t] + (lens >> 20), n0,
        &s_G[NW * wg], &s_G[(d + pad) >> 5], (d + pad) & 31, vw);
    u64 pend = 0;
#pragma unroll
    for (int k = 0; k < NW; k++) {
      pend |= static_cast<u64>(pw.w[k]) << (32 * k);
    }

    // Rare path. The screen only ever passes too much.
    while (pend != 0) {
      const int i = __ffsll(static_cast<unsigned long long>(pend)) - 1;
      pend &= pend - 1;
      scan5_after_screen<STR, ORD>(args, ctl, s_pool, s_H1[t], s_H0[t],
                                   s_abc[t], live & ~(1u << u0),
                                   s_base[t] + q0 + i, d, e0 + i);
    }
  }
  return local_eval;
}

// WIDE: the variant for pools with rows longer than SCAN5_WIDE_MIN_ROW. It
// keeps the gate-transposed pool in LDS next to the row-form pool (at the
// dense stride, to stay within a quarter of a CU's LDS) and sends every
// batch with such a row through the wide walk. The host picks the variant
// by pool size, so pools without long rows run the 48 B-stride kernel
// with no transposed pool to build.
template <bool WIDE, bool ORD>
__global__ void __launch_bounds__(SCAN_BLOCK, 4) k_scan5(ScanArgs args) {
  // Triple batching: one dequeue + one cooperative prefix-cell build + one
  // barrier per TB triples (measured at TB=1: 48% of wave time parked on
  // the per-triple barriers; batching amortizes them 8x).
  //
  // The short-row screen reads whole segments of SEG pool rows without
  // per-pair bounds tests; the pad rows keep a segment that starts at the
  // pool's last gate inside the array (their content is masked out).
  constexpr int STR = WIDE ? PSTR_DENSE : PSTR;
  constexpr int SEG = 4, LG_SEG = 2;
  // Wide walk: a task screens the 32 NW gates of NW aligned words of G
  // (geometry: sbg/scan5_geom.hpp).
  __shared__ alignas(16) u64 s_pool[(MAX_GATES + SEG) * STR];
  __shared__ alignas(16) u32 s_G[WIDE ? GT_DWORDS : 1];
  __shared__ int s_wide;         // this batch takes the wide walk
  // Wide walk: position lists of each triple's screen cell (see
  // gt_build_lists).
  __shared__ alignas(16) u8 s_pos[WIDE ? TB : 1][GT_LIST_BYTES];
  // Wide walk: all that a task needs of its triple before the G reads, in
  // one record that a wave fetches at one address in one round trip.
  // Dwords: 0 the triple's first task, 1 its task count (unpadded), 2 and 3
  // the window [lo, hi), 4 c | live << 16 | screen cell << 24, 5 the lists'
  // padded lengths and the target-0 list's offset, 10 bits each, 8..11 and
  // 12..15 the first 16 positions of the target-1 and the target-0 list.
  __shared__ alignas(16) u32 s_rec[WIDE ? TB : 1][16];
  __shared__ alignas(16) u64 s_H1[TB][8][4];
  __shared__ alignas(16) u64 s_H0[TB][8][4];
  __shared__ i64 s_base[TB];     // flat-rank base of each triple
  __shared__ i64 s_lo[TB], s_prefix[TB + 1];
  __shared__ int s_hi[TB];       // window end (flat pair index) per triple
  __shared__ int s_tpre[TB + 1]; // prefix sums of the walk's task counts
  __shared__ int s_m[TB];
  __shared__ u16 s_abc[TB][3];
  __shared__ u32 s_live[TB];     // cells with both forced-1 and forced-0
                                 // content; only these can contradict
  __shared__ u32 s_best[TB];     // (min side popcount << 3 | 7 - u) of the
                                 // most balanced live cell: the screen cell
  __shared__ i64 s_batch;        // first triple index of the batch
  __shared__ int s_stop;         // all triples past range end

  const int n = args.n;
  const int pad = scan5_wide_pad(n);  // shift of the gate ids inside G
  load_pool_lds<STR>(s_pool, args.pool, n);
  if constexpr (WIDE) {
    __syncthreads();
    // Published by the barriers of the first dequeue.
    build_gate_transposed_lds<STR>(s_G, s_pool, n, pad);
  }

  DevCtl* ctl = args.ctl;
  const i64 total3 = cf3(n);
  u64 local_eval = 0;

  for (;;) {
    const i64 batch_base =
        dequeue_batch<ORD>(ctl, TB, args.count_all, false, &s_batch);
    if (batch_base < 0) break;

    // Threads 0..TB-1 decode one triple each and compute its pair window.
    if (threadIdx.x < TB) {
      const int t = threadIdx.x;
      PrefixWindow<3> p = decode_prefix_window<3>(batch_base + t, total3, args);
      drop_dead_prefix(p, args);
      s_base[t] = p.base;
      s_lo[t] = p.lo;
      s_hi[t] = static_cast<int>(p.hi);  // <= C(m, 2) < 2^17
      s_m[t] = p.m;
      for (int j = 0; j < 3; j++) s_abc[t][j] = static_cast<u16>(p.ids[j]);
      s_prefix[t + 1] = p.hi - p.lo;  // count, turned into prefix sums below
      if (t == 0) s_prefix[0] = 0;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      // Prefix-sum the TB pair counts. Termination: triple flat-rank bases
      // increase with the triple index, so once the batch's first triple
      // is past the range end (or past the triple space), every later
      // batch is too.
      s_stop = (batch_base >= total3 || s_base[0] >= args.end) ? 1 : 0;
      // Ordered: a batch that begins above the best hit known holds nothing
      // that can lower it, and neither does any later batch.
      if constexpr (ORD) {
        if (!s_stop && static_cast<u64>(s_base[0]) > dev_best(ctl)) s_stop = 1;
      }
      // Row-segment tasks. A task is (triple, row d2, segment): the pairs
      // (d2, e2) with gap e2 - d2 - 1 in [s0, s0 + L). Segment s0 exists for
      // the rows d2 < m - 1 - s0, so a triple has sum_s (m - 1 - s * L)
      // tasks. L = SEG = 4 pairs, the flat walk's old run length: the
      // scans of the search's small pools are dominated by survivors going
      // through the solver one after another in their lane, and 8-pair
      // segments made the AES bit-0 search 15% slower than 4-pair ones.
      //
      // A batch whose longest row exceeds SCAN5_WIDE_MIN_ROW takes the wide
      // walk instead. A task there is (triple, row d, word group Wg): the
      // pairs (d, e) with e among the GB gates of G's words [NW Wg,
      // NW Wg + NW), whose ids are shifted by pad so that the pool's last
      // gate ends the last group; the ids that no gate has are the low
      // bits of group 0, which has the fewest rows. Each triple's task
      // count is padded to a multiple of 64 so that a wave never holds two
      // triples and the walk's position loop is scalar.
      int mmax = 0;
      for (int t = 0; t < TB; t++) {
        if (s_prefix[t + 1] != 0 && s_m[t] > mmax) mmax = s_m[t];
      }
      const bool wide = WIDE && mmax > SCAN5_WIDE_MIN_ROW;
      s_wide = wide ? 1 : 0;
      s_tpre[0] = 0;
      for (int t = 0; t < TB; t++) {
        int cnt = 0;
        if (s_prefix[t + 1] != 0) {
          const int rows = s_m[t] - 1;
          if (wide) {
            cnt = scan5_wide_task_count(n, pad, n - 1 - s_m[t]);
            if constexpr (WIDE) {
              s_rec[t][0] = static_cast<u32>(s_tpre[t]);
              s_rec[t][1] = static_cast<u32>(cnt);
              s_rec[t][2] = static_cast<u32>(s_lo[t]);
              s_rec[t][3] = static_cast<u32>(s_hi[t]);
            }
            cnt = (cnt + 63) & ~63;
          } else {
            const int ns = (rows + SEG - 1) >> LG_SEG;
            cnt = ns * rows - SEG * (ns * (ns - 1) / 2);
          }
        }
        s_tpre[t + 1] = s_tpre[t] + cnt;
      }
      for (int t = 0; t < TB; t++) s_prefix[t + 1] += s_prefix[t];
    }
    __syncthreads();
    if (s_stop) break;
    const i64 total_pairs = s_prefix[TB];
    if (total_pairs == 0) continue;

    build_prefix_cells<3, TB, STR>(s_pool, s_abc, s_prefix, args.T1, args.T0, s_H1,
                              s_H0);
    if (threadIdx.x < TB) s_best[threadIdx.x] = 0;
    if (mark_live_cells<3, TB>(s_H1, s_H0, s_live)) {
      // The screen runs on one cell per triple; the one whose smaller
      // side is largest rejects most (on the benchmark pool the lowest
      // live cell lets ~1.6% of candidates through, this one ~none).
      const int t = threadIdx.x >> 3;
      const int u = threadIdx.x & 7;
      int n1 = 0, n0 = 0;
      for (int w = 0; w < 4; w++) {
        n1 += __popcll(s_H1[t][u][w]);
        n0 += __popcll(s_H0[t][u][w]);
      }
      atomicMax(&s_best[t], (static_cast<u32>(n1 < n0 ? n1 : n0) << 3) |
                                static_cast<u32>(7 - u));
    }
    __syncthreads();
    if (WIDE && s_wide) {
      // 32 threads per triple list the positions of its screen cell.
      static_assert(SCAN_BLOCK == 32 * TB);
      const int t = threadIdx.x >> 5;
      if (s_prefix[t + 1] != s_prefix[t]) {  // else: cells not built
        const int u0 = 7 - static_cast<int>(s_best[t] & 7u);
        int counts[3];
        gt_build_lists(s_H1[t][u0], s_H0[t][u0], s_pos[t],
                       reinterpret_cast<u8*>(&s_rec[t][8]), counts,
                       threadIdx.x & 31);
        if ((threadIdx.x & 31) == 0) {
          s_rec[t][4] = static_cast<u32>(n - 1 - s_m[t]) | (s_live[t] << 16) |
                        (static_cast<u32>(u0) << 24);
          s_rec[t][5] = static_cast<u32>(counts[0]) |
                        (static_cast<u32>(counts[1]) << 10) |
                        (static_cast<u32>(counts[2]) << 20);
        }
      }
      __syncthreads();
    }

    const int total_tasks = s_tpre[TB];
    int since_poll = 0;

    // Wide walk (scan5_wide_walk).
    if constexpr (WIDE) {
      if (s_wide) {
        local_eval += scan5_wide_walk<STR, ORD>(
            args, ctl, pad, total_tasks, (lds_cu64*)s_pool, (lds_cu32*)s_G,
            (lds_cu32*)s_tpre, (lds_cu32*)s_rec, (lds_cu8*)s_pos,
            (lds_cu64*)s_H1, (lds_cu64*)s_H0, (lds_cu16*)s_abc,
            (lds_cu64*)s_base);
        continue;
      }
    }

    // Row-segment walk. Consecutive lanes take consecutive rows d2 of one
    // segment column: a wave mostly shares t (same-address reads of the
    // prefix cells) and its lanes read consecutive pool rows, which the
    // 48 B stride keeps conflict-free.
    constexpr int L = SEG;
    for (int task = threadIdx.x; task < total_tasks; task += blockDim.x) {
      if (!args.count_all) {
        // Abort poll once per 64 pairs walked, as the flat walk did.
        since_poll += L;
        if (since_poll >= 64) {
          since_poll = 0;
          if (!ORD && dev_abort(ctl)) break;  // ordered: see the wide walk
        }
      }
      int t = 0;
      while (s_tpre[t + 1] <= task) t++;
      const int m = s_m[t];
      int d2 = task - s_tpre[t];
      int s0 = 0;  // first gap (e2 - d2 - 1) of the segment
      for (int rows = m - 1; d2 >= rows; rows -= L) {
        d2 -= rows;
        s0 += L;
      }
      // Flat pair index of segment position 0: S(d2) + s0. Position i is
      // the pair (d2, d2 + 1 + s0 + i). Clip positions to the row's end and
      // to the triple's [lo, hi) window — per task, never per pair.
      const int q_seg = d2 * m - d2 * (d2 + 1) / 2 + s0;
      const int lo = static_cast<int>(s_lo[t]);
      const int i_lo = lo > q_seg ? lo - q_seg : 0;
      int i_hi = m - 1 - d2 - s0;
      if (i_hi > L) i_hi = L;
      if (i_hi > s_hi[t] - q_seg) i_hi = s_hi[t] - q_seg;
      if (i_lo >= i_hi) continue;
      u32 valid = ((1u << i_hi) - 1u) & ~((1u << i_lo) - 1u);  // i_hi <= SEG
      // c + 1 + d2 with c = n - 1 - m (measured: fetching c from s_abc
      // here, one more LDS read per task, cost 1% on the bench).
      const int d = n - m + d2;
      const int e_first = d + 1 + s0;  // gate at position 0
      if (args.excl != 0) {
        // An excluded d drops the whole row; excluded e's (ids < 64 only)
        // drop out of the position mask with one shift per task.
        if (dev_excluded(args.excl, d)) continue;
        if (e_first < 64) valid &= ~static_cast<u32>(args.excl >> e_first);
      }
      local_eval += __popc(valid);

      // d side, once per task: the screen cell's forced-1 / forced-0 sets
      // split by td (A = with d, N = without d), 32 registers. A cell that
      // is not live has one side empty and rejects nothing, so live == 0
      // (s_best then names cell 7) needs no special case: every pair goes
      // on to the solver, as before.
      const u32 live = s_live[t];
      const int u0 = 7 - static_cast<int>(s_best[t] & 7u);
      u32 A1[8], A0[8], N1[8], N0[8];
#pragma unroll
      for (int w = 0; w < 4; w++) {
        const u64 tdw = s_pool[d * STR + w];
        const u64 h1 = s_H1[t][u0][w], h0 = s_H0[t][u0][w];
        const u64 a1 = h1 & tdw, a0 = h0 & tdw;
        const u64 n1 = h1 ^ a1, n0 = h0 ^ a0;
        A1[2 * w] = static_cast<u32>(a1);
        A1[2 * w + 1] = static_cast<u32>(a1 >> 32);
        A0[2 * w] = static_cast<u32>(a0);
        A0[2 * w + 1] = static_cast<u32>(a0 >> 32);
        N1[2 * w] = static_cast<u32>(n1);
        N1[2 * w + 1] = static_cast<u32>(n1 >> 32);
        N0[2 * w] = static_cast<u32>(n0);
        N0[2 * w + 1] = static_cast<u32>(n0 >> 32);
      }

      // e side: one bit per position whose cell u0 has no quadrant holding
      // both forced-1 and forced-0 content. All four quadrants are tested
      // without a branch: on the benchmark pool a single quadrant rejects
      // only ~40% of the candidates (the four together ~99%), so a wave
      // almost never agrees on an early exit. No exclusion and no clipping
      // per pair; reads past the row's end are masked by `valid`.
      u32 pend = 0;
      const u64* pe = &s_pool[e_first * STR];
#pragma unroll
      for (int j = 0; j < SEG; j++) {
        // Pool rows start 16 B aligned: two ds_read_b128.
        const lds_u32x4* p =
            reinterpret_cast<const lds_u32x4*>(pe + j * STR);
        const lds_u32x4 lo4 = p[0], hi4 = p[1];
        const u32 te[8] = {lo4.x, lo4.y, lo4.z, lo4.w,
                           hi4.x, hi4.y, hi4.z, hi4.w};
        u32 x11_1 = A1[0] & te[0], x11_0 = A0[0] & te[0];
        u32 x01_1 = N1[0] & te[0], x01_0 = N0[0] & te[0];
        u32 x10_1 = A1[0] & ~te[0], x10_0 = A0[0] & ~te[0];
        u32 x00_1 = N1[0] & ~te[0], x00_0 = N0[0] & ~te[0];
#pragma unroll
        for (int k = 1; k < 8; k++) {
          x11_1 = dev_and_or(A1[k], te[k], x11_1);
          x11_0 = dev_and_or(A0[k], te[k], x11_0);
          x01_1 = dev_and_or(N1[k], te[k], x01_1);
          x01_0 = dev_and_or(N0[k], te[k], x01_0);
          x10_1 = dev_andn_or(A1[k], te[k], x10_1);
          x10_0 = dev_andn_or(A0[k], te[k], x10_0);
          x00_1 = dev_andn_or(N1[k], te[k], x00_1);
          x00_0 = dev_andn_or(N0[k], te[k], x00_0);
        }
        // min(a, b) != 0 <=> both sides non-empty; kept arithmetic so
        // the four tests do not turn into divergent branches.
        const u32 conflict = min(x11_1, x11_0) | min(x10_1, x10_0) |
                             min(x01_1, x01_0) | min(x00_1, x00_0);
        pend |= static_cast<u32>(conflict == 0) << j;
      }
      pend &= valid;

      // Rare path. The screen only ever passes too much.
      while (pend != 0) {
        const int i = __ffs(pend) - 1;
        pend &= pend - 1;
        scan5_after_screen<STR, ORD>(args, ctl, s_pool, s_H1[t], s_H0[t],
                                     s_abc[t], live & ~(1u << u0),
                                     s_base[t] + q_seg + i, d, e_first + i);
      }
    }
  }

  block_add_evaluated(ctl, local_eval);
}

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

#ifndef SBG_ORDERED_TU  // the filter has one variant: no hit ever aborts it
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
#endif  // SBG_ORDERED_TU

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

#ifdef SBG_ORDERED_TU
// ---------------------------------------------------------------------------
// Launchers of the ordered variants (scan_ordered.hpp).
// ---------------------------------------------------------------------------

void launch_ordered_scan(OrderedScan which, int grid, hipStream_t stream,
                         const void* scan_args) {
  const ScanArgs& args = *static_cast<const ScanArgs*>(scan_args);
  void (*kernel)(ScanArgs) = nullptr;
  switch (which) {
    case ORDERED_SCAN3: kernel = k_scan3<true>; break;
    case ORDERED_SCAN4: kernel = k_scan4<true>; break;
    case ORDERED_SCAN5_ROWS: kernel = k_scan5<false, true>; break;
    case ORDERED_SCAN5_WIDE: kernel = k_scan5<true, true>; break;
    case ORDERED_SCAN4S: kernel = k_scan4s<true>; break;
  }
  hipLaunchKernelGGL(kernel, dim3(grid), dim3(SCAN_BLOCK), 0, stream, args);
}

void launch_ordered_assign7(int grid, hipStream_t stream, const void* hits,
                            unsigned long long nhits, void* ctl, u64 seed) {
  hipLaunchKernelGGL(k_scan7_assign<true>, dim3(grid), dim3(SCAN_BLOCK), 0,
                     stream, static_cast<const Hit7*>(hits), nhits,
                     static_cast<DevCtl*>(ctl), seed);
}

#else  // !SBG_ORDERED_TU
// ---------------------------------------------------------------------------
// GpuEngine host wrapper.
// ---------------------------------------------------------------------------

struct GpuEngine::Impl {
  int device = 0;
  hipStream_t stream = nullptr;
  ttable* d_pool = nullptr;
  DevCtl* d_ctl = nullptr;
  Hit7* d_hits = nullptr;
  Avail3Matcher* d_matcher = nullptr;
  Pair2Stage* d_pair2 = nullptr;  // k=2: matcher and visit order
  Pair2Stage* h_pair2 = nullptr;  // pinned staging
  ttable* h_pool = nullptr;  // pinned staging: pageable-source async
                             // copies cost ~100s of us on small scans
  const Avail3Matcher* last_matcher = nullptr;  // uploaded-matcher cache
  u64 hit_cap = 0;
  DevCtl* h_ctl = nullptr;  // pinned staging
  std::string name;
  std::shared_ptr<ScanService> svc;  // lazily acquired for k=4 scans
  bool svc_tried = false;
  bool svc_broken = false;

  ~Impl() {
    // hipFree waits for the whole device, a resident service kernel
    // included: stop that kernel first, or the first hipFree below sits out
    // the service's idle limit (measured: 1.77 s per engine destroyed).
    // Other engines that share the service relaunch it on their next scan.
    if (svc != nullptr) {
      try {
        svc->park();
      } catch (const std::exception&) {
        // The kernel then retires by itself at its idle limit.
      }
      svc.reset();
    }
    if (d_pool != nullptr) (void)hipFree(d_pool);
    if (d_matcher != nullptr) (void)hipFree(d_matcher);
    if (d_pair2 != nullptr) (void)hipFree(d_pair2);
    if (h_pair2 != nullptr) (void)hipHostFree(h_pair2);
    if (d_ctl != nullptr) (void)hipFree(d_ctl);
    if (d_hits != nullptr) (void)hipFree(d_hits);
    if (h_ctl != nullptr) (void)hipHostFree(h_ctl);
    if (h_pool != nullptr) (void)hipHostFree(h_pool);
    if (stream != nullptr) (void)hipStreamDestroy(stream);
  }

  // One launch round trip: upload h_ctl, launch, download h_ctl, wait.
  template <class... Params, class... Args>
  void run(void (*kernel)(Params...), int grid, Args&&... args) {
    run_with([&] {
      hipLaunchKernelGGL(kernel, dim3(grid), dim3(SCAN_BLOCK), 0, stream,
                         static_cast<Params>(args)...);
    });
  }

  // The same round trip around any launch on `stream`.
  template <class Launch>
  void run_with(Launch launch) {
    SBG_HIP_CHECK(hipMemcpyAsync(d_ctl, h_ctl, sizeof(DevCtl),
                                 hipMemcpyHostToDevice, stream));
    launch();
    SBG_HIP_CHECK(hipGetLastError());
    SBG_HIP_CHECK(hipMemcpyAsync(h_ctl, d_ctl, sizeof(DevCtl),
                                 hipMemcpyDeviceToHost, stream));
    SBG_HIP_CHECK(hipStreamSynchronize(stream));
  }
};

// Ranks, among the np-prefixes, of the prefixes of the first and the last
// k-combination in [begin, end): the span of the kernels' prefix queue.
static void prefix_rank_span(int n, int k, int np, i64 begin, i64 end,
                             i64* first, i64* last) {
  gatenum comb[7];
  nth_combination(begin, n, k, 0, comb);
  *first = combination_rank(comb, np, n);
  nth_combination(end - 1, n, k, 0, comb);
  *last = combination_rank(comb, np, n);
}

// Ordered scans: the kernels report only the rank of the lowest hit. Its
// result words are those of the CPU scan of the single-rank window
// [rank, rank + 1), so they are the CPU's by construction. A miss there
// means kernel and CPU disagree about a candidate: that is an error, never
// a miss of the scan.
static ScanResult ordered_result(int k, const ScanRequest& rq, u64 rank,
                                 u64 evaluated) {
  const i64 r = static_cast<i64>(rank);
  ScanResult out;
  switch (k) {
    case 3: out = cpu_scan3(rq, r, r + 1); break;
    case 4: out = cpu_scan4(rq, r, r + 1); break;
    case 5: out = cpu_scan5(rq, r, r + 1); break;
    case 7: out = cpu_scan7(rq, r, r + 1); break;
    default: out = cpu_scan4s(rq, r, r + 1); break;
  }
  if (!out.found) {
    throw std::runtime_error(
        "ordered scan k=" + std::to_string(k) + ": rank " +
        std::to_string(rank) + " hits on the GPU and misses on the CPU");
  }
  out.evaluated = evaluated;
  return out;
}

bool gpu_available() { return gpu_count() > 0; }

int gpu_count() {
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess) return 0;
  return count;
}

std::unique_ptr<GpuEngine> GpuEngine::create(int device, std::string* err) {
  int count = 0;
  hipError_t e = hipGetDeviceCount(&count);
  if (e != hipSuccess || count == 0) {
    if (err != nullptr) {
      *err = e == hipSuccess ? "no HIP devices visible" : hipGetErrorString(e);
    }
    return nullptr;
  }
  try {
    auto impl = std::make_unique<Impl>();
    if (device >= 0) {
      SBG_HIP_CHECK(hipSetDevice(device));
      impl->device = device;
    } else {
      SBG_HIP_CHECK(hipGetDevice(&impl->device));
    }
    hipDeviceProp_t prop;
    SBG_HIP_CHECK(hipGetDeviceProperties(&prop, impl->device));
    impl->name = prop.name;
    SBG_HIP_CHECK(hipStreamCreate(&impl->stream));
    SBG_HIP_CHECK(hipMalloc(&impl->d_pool, sizeof(ttable) * MAX_GATES));
    SBG_HIP_CHECK(hipMalloc(&impl->d_ctl, sizeof(DevCtl)));
    SBG_HIP_CHECK(hipMalloc(&impl->d_matcher, sizeof(Avail3Matcher)));
    SBG_HIP_CHECK(hipMalloc(&impl->d_pair2, sizeof(Pair2Stage)));
    SBG_HIP_CHECK(hipHostMalloc(&impl->h_pair2, sizeof(Pair2Stage)));
    SBG_HIP_CHECK(hipHostMalloc(&impl->h_ctl, sizeof(DevCtl)));
    SBG_HIP_CHECK(hipHostMalloc(&impl->h_pool, sizeof(ttable) * MAX_GATES));
    // Hit buffer for the 7-LUT frontier: default 16M hits (768 MB) per
    // chunk; overridable for memory-constrained runs. Allocated lazily on
    // the first 7-LUT scan (gate-mode engines never need it).
    const char* cap_env = std::getenv("SBOXGATES_HIT_CAP");
    impl->hit_cap = cap_env != nullptr ? std::strtoull(cap_env, nullptr, 10)
                                       : (1ULL << 24);
    return std::unique_ptr<GpuEngine>(new GpuEngine(impl.release()));
  } catch (const std::exception& ex) {
    if (err != nullptr) *err = ex.what();
    return nullptr;
  }
}

GpuEngine::~GpuEngine() { delete impl_; }

int GpuEngine::device() const { return impl_->device; }
std::string GpuEngine::device_name() const { return impl_->name; }

bool GpuEngine::scan4_service_active() {
  Impl* im = impl_;
  if (im->svc != nullptr) return true;
  if (im->svc_broken || im->svc_tried) return false;
  im->svc_tried = true;
  const char* off = std::getenv("SBOXGATES_NO_SVC");
  if (off != nullptr && off[0] != '\0' && off[0] != '0') {
    im->svc_broken = true;
    return false;
  }
  std::string err;
  im->svc = ScanService::acquire(im->device, &err);
  if (im->svc == nullptr) {
    im->svc_broken = true;
    return false;
  }
  return true;
}

ScanResult GpuEngine::scan(int k, const ScanRequest& rq, i64 begin, i64 end) {
  ScanResult out;
  if (k == 2 && begin < 0) begin = 0;  // as cpu_scan2 does
  if (k == SCAN_SHARED && begin < 0) begin = 0;  // as cpu_scan4s does
  const i64 total = scan_space(rq.n, k);
  if (begin >= total) return out;
  if (end > total) end = total;
  if (begin >= end) return out;

  Impl* im = impl_;
  SBG_HIP_CHECK(hipSetDevice(im->device));
  // count_all ignores the option; the pair scan is ordered as it is.
  const bool ordered = rq.ordered && !rq.count_all && k != 2;

  // Service only for small/medium ranges: its 64-WG grid is sized for the
  // request/response round trip, not for multi-million-candidate scans —
  // those go to the one-shot kernel with a work-sized grid.
  if (k == 2) check_pair2_request(rq);
  if ((k == 4 || k == 2) && end - begin <= (1 << 20) && scan4_service_active()) {
    if (k == 4 && rq.matcher == nullptr) {
      throw std::runtime_error("scan4 needs matcher");
    }
    try {
      return k == 4 ? im->svc->scan4(rq, begin, end)
                    : im->svc->scan2(rq, begin, end);
    } catch (const std::exception& e) {
      // Service failure (residency/timeout): permanently fall back to the
      // one-shot launch path for this engine.
      std::fprintf(stderr, "sboxgates: scan service disabled: %s\n", e.what());
      im->svc.reset();
      im->svc_broken = true;
    }
  } else if (k != 4 && k != 2 && im->svc != nullptr) {
    // Do not let an idle-resident service delay other kernels.
    im->svc->park();
  }

  // Upload the pool (through pinned staging) and reset the control block.
  std::memcpy(im->h_pool, rq.tables, sizeof(ttable) * rq.n);
  SBG_HIP_CHECK(hipMemcpyAsync(im->d_pool, im->h_pool, sizeof(ttable) * rq.n,
                               hipMemcpyHostToDevice, im->stream));
  std::memset(im->h_ctl, 0, sizeof(DevCtl));
  if (ordered) im->h_ctl->best = ~0ULL;

  // One-shot launch of a kernel in the mode of this scan.
  const auto launch = [&](void (*kernel)(ScanArgs), OrderedScan ord, int grid,
                          const ScanArgs& a) {
    if (ordered) {
      im->run_with(
          [&] { launch_ordered_scan(ord, grid, im->stream, &a); });
    } else {
      im->run(kernel, grid, a);
    }
  };

  ScanArgs args;
  args.pool = im->d_pool;
  args.ctl = im->d_ctl;
  args.hits = im->d_hits;
  args.hit_cap = im->hit_cap;
  args.matcher = im->d_matcher;
  args.pair2 = im->d_pair2;
  args.T1 = rq.target & rq.mask;
  args.T0 = ~rq.target & rq.mask;
  args.n = rq.n;
  args.begin = begin;
  args.end = end;
  args.excl = rq.excl_low64;
  args.seed = rq.seed;
  args.count_all = rq.count_all ? 1 : 0;
  args.slices7 = 1;

  if (k == 2) {
    fill_pair2_stage(im->h_pair2, rq);
    SBG_HIP_CHECK(hipMemcpyAsync(im->d_pair2, im->h_pair2, sizeof(Pair2Stage),
                                 hipMemcpyHostToDevice, im->stream));
    im->h_ctl->best = ~0ULL;
    const i64 range = end - begin;
    const int grid = static_cast<int>(
        std::min<i64>((range + SCAN_BLOCK - 1) / SCAN_BLOCK, 4096));
    im->run(k_scan2, grid, args);
    return pair2_result(im->h_ctl->best, rq, begin, end);
  } else if (k == 3 || k == 4) {
    if (k == 4) {
      if (rq.matcher == nullptr) throw std::runtime_error("scan4 needs matcher");
      if (im->last_matcher != rq.matcher) {
        // The matcher is per-engine and immutable; upload once.
        SBG_HIP_CHECK(hipMemcpy(im->d_matcher, rq.matcher, sizeof(Avail3Matcher),
                                hipMemcpyHostToDevice));
        im->last_matcher = rq.matcher;
      }
    }
    i64 range = end - begin;
    int grid = static_cast<int>(std::min<i64>((range + SCAN_BLOCK - 1) / SCAN_BLOCK,
                                              4096));
    if (k == 3) {
      launch(k_scan3<false>, ORDERED_SCAN3, grid, args);
    } else {
      launch(k_scan4<false>, ORDERED_SCAN4, grid, args);
    }
  } else if (k == 5) {
    // Seed the triple queue at the triple containing `begin`.
    i64 t_begin, t_last;
    prefix_rank_span(rq.n, 5, 3, begin, end, &t_begin, &t_last);
    im->h_ctl->queue = static_cast<unsigned long long>(t_begin);
    // Size the grid to the triple count: small scans (deep recursion) pay
    // for pool staging per block, so an always-2048 grid costs ~10x the
    // useful work there.
    i64 tcount = t_last - t_begin + 1;
    int grid = static_cast<int>(std::min<i64>((tcount + TB - 1) / TB + 1, 2048));
    // Pools without a row longer than the crossover never take the wide
    // walk: they get the variant that has no transposed pool to build.
    if (rq.n - 3 > SCAN5_WIDE_MIN_ROW) {
      launch(k_scan5<true, false>, ORDERED_SCAN5_WIDE, grid, args);
    } else {
      launch(k_scan5<false, false>, ORDERED_SCAN5_ROWS, grid, args);
    }
  } else if (k == SCAN_SHARED) {
    // Seed the triple queue at the triple containing `begin`; grid sized to
    // the batch count, as for k=5.
    i64 t_begin, t_last;
    prefix_rank_span(rq.n, 4, 3, begin, end, &t_begin, &t_last);
    im->h_ctl->queue = static_cast<unsigned long long>(t_begin);
    const i64 tcount = t_last - t_begin + 1;
    const int grid =
        static_cast<int>(std::min<i64>((tcount + SB - 1) / SB + 1, 2048));
    launch(k_scan4s<false>, ORDERED_SCAN4S, grid, args);
  } else if (k == 7) {
    if (im->d_hits == nullptr) {
      SBG_HIP_CHECK(hipMalloc(&im->d_hits, sizeof(Hit7) * im->hit_cap));
      // args was built before the allocation; refresh the pointer.
    }
    args.hits = im->d_hits;
    // Filter + assign, with overflow-driven range splitting.
    i64 lo = begin;
    while (lo < end) {
      i64 hi = end;
      for (;;) {
        std::memset(im->h_ctl, 0, sizeof(DevCtl));
        if (ordered) {
          im->h_ctl->best = ~0ULL;
          im->h_ctl->pool_n = static_cast<u32>(rq.n);
        }
        i64 q_begin, q_last;
        prefix_rank_span(rq.n, 7, 4, lo, hi, &q_begin, &q_last);
        i64 qcount = q_last - q_begin + 1;
        // Sub-quad slicing: a single quad prefix can hold C(n-4,3) triples
        // (tens of thousands); without slicing a small scan runs on a
        // handful of blocks and leaves the chip idle.
        i64 want_units = (hi - lo + SLICE_UNIT - 1) / SLICE_UNIT;
        int slices = static_cast<int>(
            std::clamp<i64>(want_units / std::max<i64>(qcount, 1), 1, 256));
        ScanArgs a2 = args;
        a2.begin = lo;
        a2.end = hi;
        a2.slices7 = slices;
        im->h_ctl->queue = static_cast<unsigned long long>(q_begin * slices);
        int grid7 = static_cast<int>(
            std::min<i64>((qcount * slices + QB - 1) / QB + 1, 2048));
        im->run(k_scan7_filter, grid7, a2);
        if (im->h_ctl->overflow == 0) break;
        // Too many feasible combinations for the buffer: halve the range.
        hi = lo + (hi - lo) / 2;
        if (hi <= lo + 1) {
          throw std::runtime_error("7-LUT hit buffer too small for one combo");
        }
      }
      // Accounting invariant: h_ctl is zeroed at the top of every attempt,
      // so only the final (non-overflowed) attempt's counter lands here —
      // combinations re-scanned after an overflow are never double-counted.
      out.evaluated += im->h_ctl->evaluated;
      unsigned long long nhits = im->h_ctl->hit_count;
      if (nhits > im->hit_cap) nhits = im->hit_cap;
      if (nhits > 0 && !rq.count_all) {
        u64 items = nhits * LUT7_NUM_ORDERINGS * FM_SPLIT;
        int grid = static_cast<int>(
            std::min<u64>((items + SCAN_BLOCK - 1) / SCAN_BLOCK, 4096));
        // h_ctl still holds the filter's final state, which the upload
        // puts back unchanged.
        if (ordered) {
          im->run_with([&] {
            launch_ordered_assign7(grid, im->stream, im->d_hits, nhits,
                                   im->d_ctl, rq.seed);
          });
        } else {
          im->run(k_scan7_assign<false>, grid, im->d_hits, nhits, im->d_ctl,
                  rq.seed);
        }
        // Ordered: the sub-ranges come in increasing order, so the first one
        // with a hit holds the scan's lowest.
        if (ordered && im->h_ctl->best != ~0ULL) {
          return ordered_result(7, rq, im->h_ctl->best, out.evaluated);
        }
        if (im->h_ctl->found != 0) {
          out.found = true;
          std::memcpy(out.res, im->h_ctl->res, sizeof(out.res));
          return out;
        }
      }
      lo = hi;
    }
    return out;
  } else {
    throw std::runtime_error("GpuEngine::scan: bad k");
  }

  out.evaluated = im->h_ctl->evaluated;
  if (ordered && im->h_ctl->best != ~0ULL) {
    const u64 best = im->h_ctl->best;
    return ordered_result(k, rq, k <= 4 ? best >> BEST3_SHIFT : best,
                          out.evaluated);
  }
  if (im->h_ctl->found != 0) {
    out.found = true;
    std::memcpy(out.res, im->h_ctl->res, sizeof(out.res));
  }
  return out;
}

#endif  // SBG_ORDERED_TU

}  // namespace sbg
