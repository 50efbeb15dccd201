// scan5.hpp — the 5-LUT scan kernel k_scan5 with what only it uses: the
// gate-transposed pool and its per-position cell test (gt_*), the survivor
// routine, the wide walk and its wave-owned variant k_scan5_wave. Included
// by the kernel modules only
// (scan_launch.hpp).
#pragma once

#include "sbg/scan5_cell.hpp"
#include "sbg/scan5_geom.hpp"
#include "scan_device.hpp"

namespace sbg {
namespace {

// ---------------------------------------------------------------------------
// Gate-transposed pool. G[p][W], p a truth-table position and W a 32-gate
// word: bit i of G[p][W] is bit p of the gate with shifted id 32 W + i,
// i.e. of gate 32 W + i - pad (0 where that is no gate of the pool). The
// caller chooses pad so that the pool's last gate ends a word group (see
// sbg/scan5_geom.hpp); n + pad <= 32 GT_WORDS. One
// dword then holds one table position of 32 candidates' last gate, and a
// cell test over those candidates costs a few instructions per position of
// the cell instead of a pass over whole 256-bit tables per candidate.
// ---------------------------------------------------------------------------
constexpr int GT_WORDS = (MAX_GATES + 31) / 32;  // dwords per position
constexpr int GT_DWORDS = 256 * GT_WORDS;

// 16- and 8-byte LDS reads of u64 / u32 arrays through another type
// (may_alias makes the differently-typed read well defined).
typedef u32 lds_u32x4 __attribute__((ext_vector_type(4), may_alias, aligned(16)));
typedef u32 lds_u32x2 __attribute__((ext_vector_type(2), may_alias, aligned(8)));
typedef u32 lds_u32 __attribute__((may_alias));

// Cooperative build of G in LDS from the row-form pool staged at stride STR
// (call after the barrier that publishes s_pool; the caller places the one
// that publishes s_G). A wave takes 64 gates and one 32-position table
// word at a time: lane = gate, one ballot per position, lane b keeps
// position b's 64 gate bits and stores them as two dwords.
template <int STR>
__device__ __forceinline__ void build_gate_transposed_lds(u32* s_G,
                                                          const u64* s_pool,
                                                          int n, int pad) {
  const int lane = threadIdx.x & 63;
  const int nwaves = blockDim.x >> 6;
  const int items = ((n + pad + 63) >> 6) * 8;  // (64-id chunk, table word)
  for (int item = threadIdx.x >> 6; item < items; item += nwaves) {
    const int chunk = item >> 3, w = item & 7;
    const int gate = chunk * 64 + lane - pad;
    u32 row = 0;
    if (gate >= 0 && gate < n) {
      row = reinterpret_cast<const lds_u32*>(&s_pool[gate * STR])[w];
    }
    u32 lo = 0, hi = 0;
#pragma unroll
    for (int b = 0; b < 32; b++) {
      const u64 bal = __ballot((row >> b) & 1u);
      if (lane == b) {
        lo = static_cast<u32>(bal);
        hi = static_cast<u32>(bal >> 32);
      }
    }
    if (lane < 32) {
      u32* dst = &s_G[(w * 32 + lane) * GT_WORDS + 2 * chunk];
      dst[0] = lo;
      dst[1] = hi;
    }
  }
}

// G[p][W .. W + NW) for NW in {1, 2}, W even when NW == 2; gw = &G[0][W].
template <int NW>
struct GtWords {
  u32 w[NW];
};
template <int NW>
__device__ __forceinline__ GtWords<NW> gt_load(const u32* gw, u32 p) {
  static_assert(NW == 1 || NW == 2);
  GtWords<NW> g;
  if constexpr (NW == 1) {
    g.w[0] = gw[p * GT_WORDS];
  } else {
    const lds_u32x2 v = *reinterpret_cast<const lds_u32x2*>(&gw[p * GT_WORDS]);
    g.w[0] = v.x;
    g.w[1] = v.y;
  }
  return g;
}

// (a & b) | acc in one VALU instruction. Written out because the compiler
// rebalances a plain C chain of these into v_and_b32 pairs feeding
// v_or3_b32 (11 instructions per 8-dword reduction instead of 8) and keeps
// vectorized copies of the loop-invariant operands.
__device__ __forceinline__ u32 dev_and_or(u32 a, u32 b, u32 acc) {
  u32 r;
  asm("v_and_or_b32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(acc));
  return r;
}

// (a & ~b) | acc, likewise one instruction (gfx950's three-input bit op,
// truth table 0xba), so ~b is never materialised.
__device__ __forceinline__ u32 dev_andn_or(u32 a, u32 b, u32 acc) {
  u32 r;
  asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xba"
      : "=v"(r) : "v"(a), "v"(b), "v"(acc));
  return r;
}

// (~a & ~b) | acc (truth table 0xab).
__device__ __forceinline__ u32 dev_nor_or(u32 a, u32 b, u32 acc) {
  u32 r;
  asm("v_bitop3_b32 %0, %1, %2, %3 bitop3:0xab"
      : "=v"(r) : "v"(a), "v"(b), "v"(acc));
  return r;
}

// The positions of one forced side (target-1 or target-0) of a cell, seen
// by 32 NW candidates (x, e) at once, e the word's gates: per quadrant
// (x's bit, e's bit) the candidates that have one of the side's positions
// there.
template <int NW>
struct GtSide {
  u32 q11[NW] = {}, q10[NW] = {}, q01[NW] = {}, q00[NW] = {};
};

// One position: g = G[p][W ..], m = all-ones where the lane's own gate x
// has bit p set, else 0.
template <int NW>
__device__ __forceinline__ void gt_accumulate(GtSide<NW>& s,
                                              const GtWords<NW>& g, u32 m) {
#pragma unroll
  for (int k = 0; k < NW; k++) {
    s.q11[k] = dev_and_or(g.w[k], m, s.q11[k]);
    s.q10[k] = dev_andn_or(m, g.w[k], s.q10[k]);
    s.q01[k] = dev_andn_or(g.w[k], m, s.q01[k]);
    s.q00[k] = dev_nor_or(g.w[k], m, s.q00[k]);
  }
}

// Position lists of a cell's two forced sides, for gt_screen: the
// side's positions in ascending order as bytes, padded to a multiple of
// GT_LIST_STEP by repeating the last one (accumulating a position twice
// changes nothing). The target-1 list starts at byte 0, the target-0 list
// at the next multiple of 16; both are read 16 bytes at a time. The first
// GT_HEAD_BYTES of each list are filed a second time, side by side (target-1
// at byte 0, target-0 at byte GT_HEAD_BYTES of `head`), for a reader that
// wants them next to its other per-cell data; bytes past a list's padded
// length are left as they were.
constexpr int GT_LIST_STEP = 4;
constexpr int GT_LIST_BYTES = 256 + 2 * 16;
constexpr int GT_HEAD_BYTES = 16;

// Called by 32 threads, part = 0..31, each filing the 8 positions of byte
// `part` of the cell's forced sets (h1, h0: 4 words each, disjoint).
// counts[0], counts[1]: the lists' padded lengths; counts[2]: the target-0
// list's byte offset.
__device__ __forceinline__ void gt_build_lists(const u64* h1, const u64* h0,
                                               u8* list, u8* head,
                                               int* counts, int part) {
  const int wd = part >> 3, sh = (part & 7) * 8;
  int base = 0;
  for (int side = 0; side < 2; side++) {
    const u64* h = side == 0 ? h1 : h0;
    int total = 0, at = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int c = __popcll(h[k]);
      total += c;
      if (k < wd) at += c;
    }
    at += __popcll(h[wd] & ((1ULL << sh) - 1));
    const int padded = (total + GT_LIST_STEP - 1) & ~(GT_LIST_STEP - 1);
    u32 mine = static_cast<u32>(h[wd] >> sh) & 0xffu;
    if (mine != 0) {
      int p = 0;
      for (; mine != 0; mine &= mine - 1) {
        p = part * 8 + __ffs(mine) - 1;
        if (at < GT_HEAD_BYTES) {
          head[side * GT_HEAD_BYTES + at] = static_cast<u8>(p);
        }
        list[base + at++] = static_cast<u8>(p);
      }
      if (at == total) {  // the side's last position is here: pad with it
        for (; at < padded; at++) {
          if (at < GT_HEAD_BYTES) {
            head[side * GT_HEAD_BYTES + at] = static_cast<u8>(p);
          }
          list[base + at] = static_cast<u8>(p);
        }
      }
    }
    if (part == 0) counts[side] = padded;
    base = (total + 15) & ~15;
    if (part == 0 && side == 0) counts[2] = base;
  }
}

// Candidates of word k in whose cell some quadrant holds both target-1 and
// target-0 positions: no function of (cell, x, e) realises the target.
template <int NW>
__device__ __forceinline__ u32 gt_conflict(const GtSide<NW>& s1,
                                           const GtSide<NW>& s0, int k) {
  u32 c = s1.q11[k] & s0.q11[k];
  c = dev_and_or(s1.q10[k], s0.q10[k], c);
  c = dev_and_or(s1.q01[k], s0.q01[k], c);
  return dev_and_or(s1.q00[k], s0.q00[k], c);
}

// GT_LIST_STEP listed positions, the bytes of pw.
template <int NW>
__device__ __forceinline__ void gt_accumulate_step(GtSide<NW>& s, u32 pw,
                                                   const u32* gw,
                                                   const u32* gx, u32 xbit) {
#pragma unroll
  for (int i = 0; i < GT_LIST_STEP; i++) {
    const u32 p = (pw >> (8 * i)) & 0xffu;
    const GtWords<NW> g = gt_load<NW>(gw, p);
    const u32 m = static_cast<u32>(
        __builtin_amdgcn_sbfe(static_cast<int>(gx[p * GT_WORDS]), xbit, 1));
    gt_accumulate<NW>(s, g, m);
  }
}

// Screen the candidates `valid` of a wave's lanes against one cell, given
// as its two position lists (n1, n0: padded lengths; lists and lengths
// wave-uniform). gw = &G[0][W] of the lane's candidate words; x's bits
// come out of G as well: gx = &G[0][x >> 5], xbit = x & 31. Returns the
// candidates without a conflict. The lists are walked side by side,
// GT_LIST_STEP positions of each at a time, and the walk ends as soon as
// no lane of the wave has a candidate left: a few positions of either side
// already contradict nearly every candidate (sampled on the benchmark
// pool: of 60000, 1518 passed the first 4 of each side, 69 the first 6, 3
// the first 8 and none the first 12, against 104 positions in the cell), so
// the cost follows that number and not the cell's size. The list bytes go through
// SGPRs; only the G reads, the bit extract and the accumulation are
// vector work. head1, head0: the lists' first GT_HEAD_BYTES, already in
// scalars (gt_build_lists' `head`), so that the first G reads wait for no
// list read. Call from code that the whole wave runs together.
// past_heads() runs before every read of list1 / list0, which happens only
// when a side is longer than its head and the walk gets that far: a caller
// that builds the lists on demand does it there.
struct GtListsReady {
  __device__ __forceinline__ void operator()() const {}
};
template <int NW, class PastHeads = GtListsReady>
__device__ __forceinline__ GtWords<NW> gt_screen(const u32 (&head1)[4],
                                                 const u32 (&head0)[4],
                                                 const u8* list1, int n1,
                                                 const u8* list0, int n0,
                                                 const u32* gw, const u32* gx,
                                                 u32 xbit,
                                                 const GtWords<NW>& valid,
                                                 PastHeads past_heads = {}) {
  static_assert(GT_LIST_STEP == 4);  // one dword of list bytes per step
  static_assert(GT_HEAD_BYTES == 16);  // one pass of the loop below
  GtWords<NW> pend = valid;
  // An empty side cannot contradict: everything passes.
  if (n1 == 0 || n0 == 0) return pend;
  GtSide<NW> s1, s0;
  const int nmax = n1 > n0 ? n1 : n0;
  const auto remaining = [&]() {
    u32 left = 0;
#pragma unroll
    for (int w = 0; w < NW; w++) {
      pend.w[w] = valid.w[w] & ~gt_conflict<NW>(s1, s0, w);
      left |= pend.w[w];
    }
    return left;
  };
  for (int k = 0; k < nmax; k += 16) {
    u32 pw1[4] = {}, pw0[4] = {};
    if (k == 0) {
#pragma unroll
      for (int j = 0; j < 4; j++) {
        pw1[j] = head1[j];
        pw0[j] = head0[j];
      }
    } else {
      past_heads();
      if (k < n1) {
        const lds_u32x4 v = *reinterpret_cast<const lds_u32x4*>(list1 + k);
        pw1[0] = __builtin_amdgcn_readfirstlane(v.x);
        pw1[1] = __builtin_amdgcn_readfirstlane(v.y);
        pw1[2] = __builtin_amdgcn_readfirstlane(v.z);
        pw1[3] = __builtin_amdgcn_readfirstlane(v.w);
      }
      if (k < n0) {
        const lds_u32x4 v = *reinterpret_cast<const lds_u32x4*>(list0 + k);
        pw0[0] = __builtin_amdgcn_readfirstlane(v.x);
        pw0[1] = __builtin_amdgcn_readfirstlane(v.y);
        pw0[2] = __builtin_amdgcn_readfirstlane(v.z);
        pw0[3] = __builtin_amdgcn_readfirstlane(v.w);
      }
    }
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int kk = k + GT_LIST_STEP * j;
      if (kk >= nmax) break;
      if (kk < n1) gt_accumulate_step<NW>(s1, pw1[j], gw, gx, xbit);
      if (kk < n0) gt_accumulate_step<NW>(s0, pw0[j], gw, gx, xbit);
      // No test after the first step: 4 positions a side still let
      // 2.5% through, and a wave holds thousands of candidates.
      if (kk == 0) continue;
      if (!__any(remaining() != 0)) return pend;
    }
  }
  remaining();
  return pend;
}

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

// gt_build_lists by one whole wave, both sides at once, lane = 32 side +
// part: each lane files the 8
// positions of byte `part` of its side of the cell's forced sets (h1, h0: 4
// words each, disjoint). No heads: k_scan5_wave has them in registers
// (scan5_side_head). The lists' padded lengths are those of gt_build_lists:
// the side's size rounded up to GT_LIST_STEP, the target-0 list at the next
// multiple of 16 behind the target-1 list.
__device__ __forceinline__ void gt_build_lists_wave(const u64* h1,
                                                    const u64* h0, u8* list,
                                                    int lane) {
  const int side = lane >> 5, part = lane & 31;
  const int wd = part >> 3, sh = (part & 7) * 8;
  const u64* h = side == 0 ? h1 : h0;
  int total1 = 0, total0 = 0, at = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int c1 = __popcll(h1[k]), c0 = __popcll(h0[k]);
    total1 += c1;
    total0 += c0;
    if (k < wd) at += side == 0 ? c1 : c0;
  }
  const u64 hw = h[wd];
  at += __popcll(hw & ((1ULL << sh) - 1));
  const int total = side == 0 ? total1 : total0;
  const int off0 = (total1 + 15) & ~15;
  const int base = side == 0 ? 0 : off0;
  const int padded = (total + GT_LIST_STEP - 1) & ~(GT_LIST_STEP - 1);
  u32 mine = static_cast<u32>(hw >> sh) & 0xffu;
  if (mine != 0) {
    int p = 0;
    for (; mine != 0; mine &= mine - 1) {
      p = part * 8 + __ffs(mine) - 1;
      list[base + at++] = static_cast<u8>(p);
    }
    if (at == total) {  // the side's last position is here: pad with it
      for (; at < padded; at++) list[base + at] = static_cast<u8>(p);
    }
  }
}


// ---------------------------------------------------------------------------
// k_scan5_wave: a wave owns its triples. The block stages the pool and
// builds G once; from then on its waves run on their own and meet again
// only to add up `evaluated`. A wave takes a chunk of consecutive triples
// off the queue with one atomic (sbg/scan5_geom.hpp has the chunk rule) and
// sets them all up at once, one triple per lane (sbg/scan5_cell.hpp): the
// triple's ids and pair window, the sizes of its eight prefix cells, the
// live cells, the screen cell and the first GT_HEAD_BYTES positions of the
// screen cell's two sides. The walk (scan5_wave_walk, one call per chunk)
// takes a triple's values out of its lane with v_readlane and keeps them in
// scalars for the whole triple. What only the rare path reads (all eight
// prefix cells, the prefix's gate ids) and what only a long screen reads
// (the complete position lists) is built by the whole wave the first time
// a triple needs it, in a slice of LDS that only this wave touches.
// ---------------------------------------------------------------------------

// A wave's private LDS, filled on demand for the triple it is walking: the
// prefix cells and the prefix's gate ids (for the rare path) and the screen
// cell's position lists (for a screen that goes past the heads).
struct alignas(16) Scan5WaveSlice {
  u64 H1[8][4];
  u64 H0[8][4];
  u8 pos[GT_LIST_BYTES];
  u16 abc[8];  // 3 used
};

typedef __attribute__((address_space(3))) Scan5WaveSlice lds_slice;

// Set in scan5_wave_walk's result: the wave's scan ends here (aborted, or
// ordered and past the best hit known).
constexpr u64 SCAN5_WALK_STOP = 1ULL << 63;

// The rare path of a step: the pairs `pend` of row d that passed the screen
// (bit i: the pair (d, e0 + i) of flat rank rank0 + i) go through the other
// live cells and the solver. Not inlined, to keep its registers out of the
// walk's.
template <int STR, bool ORD>
__device__ __attribute__((noinline)) void scan5_wave_rare(
    const ScanArgs& args, DevCtl* ctl, lds_cu64* l_pool, lds_slice* l_slice,
    u32 other_live, i64 rank0, int d, int e0, u64 pend) {
  const u64* s_pool = (const u64*)l_pool;
  const Scan5WaveSlice* sl = (const Scan5WaveSlice*)l_slice;
  while (pend != 0) {
    const int i = __ffsll(static_cast<unsigned long long>(pend)) - 1;
    pend &= pend - 1;
    scan5_after_screen<STR, ORD>(args, ctl, s_pool, sl->H1, sl->H0, sl->abc,
                                 other_live, rank0 + i, d, e0 + i);
  }
}

// What the chunk set-up leaves for the walk in lane i about triple i. Packed
// `cells`: live cells | screen cell << 8 | size of its target-1 side << 12 |
// size of its target-0 side << 21 (sizes are at most 256).
static_assert(GT_HEAD_BYTES == SCAN5_HEAD_BYTES);
struct Scan5WaveTriple {
  int ab, c, lo, hi, base_lo, base_hi, cells;
  u32 head1[4], head0[4];
};

// Walk of one chunk's live triples (`todo`: their lanes) by one wave:
// returns the pairs this lane evaluated, with SCAN5_WALK_STOP if the wave's
// scan ends. Every argument but `todo` and the LDS arrays is per lane (v.*
// of lane i describe triple i); a triple's values go through v_readlane
// into scalars. Not inlined: inside the kernel the step loop's invariants
// were spilled and reloaded from scratch in every step; as a function it
// gets registers of its own.
template <int STR, bool ORD>
__device__ __attribute__((noinline)) u64 scan5_wave_walk(
    const ScanArgs& args, DevCtl* ctl, int pad, lds_cu64* l_pool,
    lds_cu32* l_G, lds_cu32* l_T, lds_slice* l_slice, u64 todo_, int v_ab,
    int v_c, int v_lo, int v_hi, int v_base_lo, int v_base_hi, int v_cells,
    u32 v_h10, u32 v_h11, u32 v_h12, u32 v_h13, u32 v_h00, u32 v_h01,
    u32 v_h02, u32 v_h03) {
  constexpr int NW = SCAN5_WIDE_WORDS;
  constexpr int GB = SCAN5_WIDE_GB;
  static_assert(GB == 64);  // a lane a row
  const u64* s_pool = (const u64*)l_pool;
  const u32* s_G = (const u32*)l_G;
  Scan5WaveSlice* sl = (Scan5WaveSlice*)l_slice;
  const int lane = threadIdx.x & 63;
  // Through scalars, so that the per-lane arguments get the registers.
  pad = static_cast<int>(dev_uniform(static_cast<u32>(pad)));
  const int n = static_cast<int>(dev_uniform(static_cast<u32>(args.n)));
  const int count_all =
      static_cast<int>(dev_uniform(static_cast<u32>(args.count_all)));
  const u64 excl = dev_uniform64(args.excl);
  u64 local_eval = 0;
  u64 todo = dev_uniform64(todo_);

  for (; todo != 0; todo &= todo - 1) {
    const int j = __ffsll(static_cast<unsigned long long>(todo)) - 1;
    const int ab = wave_lane_value(v_ab, j);
    const int a = ab & 0xffff, b = ab >> 16;
    const int c = wave_lane_value(v_c, j);
    const int lo = wave_lane_value(v_lo, j);
    const int hi = wave_lane_value(v_hi, j);
    const i64 base = static_cast<i64>(
        static_cast<u64>(static_cast<u32>(wave_lane_value(v_base_lo, j))) |
        static_cast<u64>(static_cast<u32>(wave_lane_value(v_base_hi, j)))
            << 32);
    // Ordered: ranks rise with the triple index, so a triple that begins
    // above the best hit known ends this wave's scan. A triple it has
    // begun runs to its end.
    if constexpr (ORD) {
      if (!count_all && static_cast<u64>(base) > wave_best(ctl)) {
        return local_eval | SCAN5_WALK_STOP;
      }
    }
    const u32 cells = static_cast<u32>(wave_lane_value(v_cells, j));
    const u32 live = cells & 0xffu;
    const int u0 = static_cast<int>((cells >> 8) & 7u);
    const int c1 = static_cast<int>((cells >> 12) & 0x1ffu);
    const int c0 = static_cast<int>(cells >> 21);
    const int n1 = (c1 + GT_LIST_STEP - 1) & ~(GT_LIST_STEP - 1);
    const int n0 = (c0 + GT_LIST_STEP - 1) & ~(GT_LIST_STEP - 1);
    const u8* list0 = sl->pos + ((c1 + 15) & ~15);
    const u32 head1[4] = {
        static_cast<u32>(wave_lane_value(static_cast<int>(v_h10), j)),
        static_cast<u32>(wave_lane_value(static_cast<int>(v_h11), j)),
        static_cast<u32>(wave_lane_value(static_cast<int>(v_h12), j)),
        static_cast<u32>(wave_lane_value(static_cast<int>(v_h13), j))};
    const u32 head0[4] = {
        static_cast<u32>(wave_lane_value(static_cast<int>(v_h00), j)),
        static_cast<u32>(wave_lane_value(static_cast<int>(v_h01), j)),
        static_cast<u32>(wave_lane_value(static_cast<int>(v_h02), j)),
        static_cast<u32>(wave_lane_value(static_cast<int>(v_h03), j))};

    // On demand, by the whole wave, at most once per triple. The syncs on
    // either side order the build against the reads of the triple before
    // and against its own readers.
    bool cells_built = false, lists_built = false;
    // The eight prefix cells, masked with target-1 / target-0, and the
    // prefix's ids: lane = (cell u = lane & 7, dword = lane >> 3).
    const auto need_cells = [&]() {
      if (cells_built) return;
      cells_built = true;
      wave_lds_sync();
      const int cu = lane & 7, cdw = lane >> 3;
      const lds_u32* pool32 = reinterpret_cast<const lds_u32*>(s_pool);
      const u32 cell = scan5_cell_dword(pool32[a * (2 * STR) + cdw],
                                        pool32[b * (2 * STR) + cdw],
                                        pool32[c * (2 * STR) + cdw], cu);
      reinterpret_cast<lds_u32*>(&sl->H1[0][0])[cu * 8 + cdw] =
          cell & l_T[cdw];
      reinterpret_cast<lds_u32*>(&sl->H0[0][0])[cu * 8 + cdw] =
          cell & l_T[8 + cdw];
      if (lane == 0) {
        sl->abc[0] = static_cast<u16>(a);
        sl->abc[1] = static_cast<u16>(b);
        sl->abc[2] = static_cast<u16>(c);
      }
      wave_lds_sync();
    };
    // The screen cell's complete position lists.
    const auto need_lists = [&]() {
      if (lists_built) return;
      lists_built = true;
      need_cells();
      gt_build_lists_wave(sl->H1[u0], sl->H0[u0], sl->pos, lane);
      wave_lds_sync();
    };

    // Walk. A task is (row d, word group): the pairs (d, e) with e among
    // the GB gates of G's words [NW wg, NW wg + NW). The tasks run through
    // the groups from the last one down, consecutive rows on consecutive
    // lanes, 64 tasks a step: (wg, row0) is the step's first task, and a
    // lane whose row lies past the group's end is in the next group down
    // (which has 64 rows fewer, or is the triple's last).
    const Scan5WideGroups g = scan5_wide_groups(n, pad, c);
    int wg = g.w_max, rows = n - 2 - c, row0 = 0;
    while (wg >= g.w_min) {
      // Unordered first-hit scans poll once per step, as often per pair
      // walked as the tasks of the batch walk did.
      if (!ORD && !count_all && wave_abort(ctl)) {
        return local_eval | SCAN5_WALK_STOP;
      }
      const int rows_down = scan5_wide_rows(pad, c, wg - 1);
      int d2 = row0 + lane, lwg = wg;
      bool mine = true;
      if (d2 >= rows) {
        d2 -= rows;
        lwg = wg - 1;
        mine = lwg >= g.w_min && d2 < rows_down;
      }
      if (!mine) {  // no task: any address inside G will do
        d2 = 0;
        lwg = wg;
      }
      // Bit i of the task is the pair (d, e0 + i), flat index q0 + i;
      // valid: clipped to e > d and to the triple's [lo, hi) window,
      // without the excluded gates.
      const Scan5WideTask wt = scan5_wide_task_at(n, pad, c, lwg, d2);
      const u64 valid = mine ? scan5_wide_valid(wt, lo, hi, excl) : 0;
      row0 += 64;
      while (wg >= g.w_min && row0 >= rows) {
        row0 -= rows;
        wg--;
        rows = scan5_wide_rows(pad, c, wg);
      }
      if (!__any(valid != 0)) continue;
      local_eval += __popcll(valid);

      // Screen: the listed positions of the screen cell. Per position the
      // lanes read G at their candidate words (the same address across
      // most of a wave: LDS broadcast) and at d's own word for td's bit.
      GtWords<NW> vw;
#pragma unroll
      for (int w = 0; w < NW; w++) {
        vw.w[w] = static_cast<u32>(valid >> (32 * w));
      }
      const GtWords<NW> pw = gt_screen<NW>(
          head1, head0, sl->pos, n1, list0, n0, &s_G[NW * wt.wg],
          &s_G[(wt.d + pad) >> 5], (wt.d + pad) & 31, vw, need_lists);
      u64 pend = 0;
#pragma unroll
      for (int w = 0; w < NW; w++) {
        pend |= static_cast<u64>(pw.w[w]) << (32 * w);
      }

      // Rare path. The screen only ever passes too much.
      if (!__any(pend != 0)) continue;
      need_cells();
      scan5_wave_rare<STR, ORD>(args, ctl, l_pool, l_slice,
                                live & ~(1u << u0), base + wt.q0, wt.d, wt.e0,
                                pend);
    }
  }
  return local_eval;
}

// Eight dwords of a pool row, two 16-byte LDS reads (rows are 32 B apart).
template <int STR>
__device__ __forceinline__ void scan5_load_row(const u64* s_pool, int id,
                                               u32 (&r)[8]) {
  static_assert(STR == PSTR_DENSE);
  const lds_u32x4* q = reinterpret_cast<const lds_u32x4*>(&s_pool[id * STR]);
  const lds_u32x4 x = q[0], y = q[1];
  r[0] = x.x; r[1] = x.y; r[2] = x.z; r[3] = x.w;
  r[4] = y.x; r[5] = y.y; r[6] = y.z; r[7] = y.w;
}

// q_begin, q_units: the first triple of the queue and the number of triples
// in it; ctl->queue counts chunks of them, from 0.
template <bool ORD>
__device__ __forceinline__ void scan5_wave_scan(const ScanArgs& args,
                                                i64 q_begin, i64 q_units) {
  constexpr int STR = PSTR_DENSE;
  static_assert(SCAN5_CHUNK_MAX == 64);  // a lane a triple
  __shared__ alignas(16) u64 s_pool[MAX_GATES * STR];
  __shared__ alignas(16) u32 s_G[GT_DWORDS];
  __shared__ Scan5WaveSlice s_slice[SCAN_BLOCK / 64];
  // T1 and T0 for the on-demand cell build, which reads them as 16 dwords
  // indexed by lane: dword w of T1 at [w], of T0 at [8 + w] (dword 2 k is
  // the low half of word k).
  __shared__ u64 s_T[2][4];

  const int n = args.n;
  const int pad = scan5_wide_pad(n);  // shift of the gate ids inside G
  load_pool_lds<STR>(s_pool, args.pool, n);
  if (threadIdx.x == 0) {
    for (int w = 0; w < 4; w++) {
      s_T[0][w] = args.T1.w[w];
      s_T[1][w] = args.T0.w[w];
    }
  }
  __syncthreads();
  build_gate_transposed_lds<STR>(s_G, s_pool, n, pad);
  __syncthreads();

  DevCtl* ctl = args.ctl;
  const int lane = threadIdx.x & 63;
  Scan5WaveSlice* sl = &s_slice[threadIdx.x >> 6];
  const int count_all = args.count_all;
  const i64 total3 = cf3(n);
  const Scan5ChunkPlan plan = scan5_chunk_plan(
      q_units, static_cast<int>(gridDim.x) * (SCAN_BLOCK / 64));
  u32 T1[8], T0[8];  // wave-uniform: kernel arguments
#pragma unroll
  for (int w = 0; w < 4; w++) {
    T1[2 * w] = static_cast<u32>(args.T1.w[w]);
    T1[2 * w + 1] = static_cast<u32>(args.T1.w[w] >> 32);
    T0[2 * w] = static_cast<u32>(args.T0.w[w]);
    T0[2 * w + 1] = static_cast<u32>(args.T0.w[w] >> 32);
  }
  u64 local_eval = 0;

  for (;;) {
    // Dequeue: one lane, one atomic per chunk. Ordered: a known hit takes
    // the abort flag's place; chunks come in increasing triple order, so
    // every chunk not yet taken ranks above any hit already known.
    int k_lo = 0, k_hi = 0;
    if (lane == 0) {
      const bool halt =
          !count_all && (ORD ? dev_best(ctl) != ~0ULL : dev_abort(ctl));
      const i64 k = halt ? -1
                         : static_cast<i64>(__hip_atomic_fetch_add(
                               &ctl->queue, 1ULL, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT));
      k_lo = static_cast<int>(k);
      k_hi = static_cast<int>(k >> 32);
    }
    const i64 k = static_cast<i64>(
        static_cast<u64>(dev_uniform(static_cast<u32>(k_lo))) |
        static_cast<u64>(dev_uniform(static_cast<u32>(k_hi))) << 32);
    if (k < 0) break;
    const Scan5Chunk ch = scan5_chunk(plan, k);
    if (ch.count == 0) break;

    // Lane i sets up triple i of the chunk: ids and pair window, then, if
    // the window is not empty, the cell sizes, the live cells, the screen
    // cell and the heads of its two position lists.
    PrefixWindow<3> p;
    if (lane < ch.count) {
      p = decode_prefix_window<3>(q_begin + ch.first + lane, total3, args);
      drop_dead_prefix(p, args);
    }
    const bool alive = p.lo < p.hi;
    Scan5WaveTriple v = {};
    v.ab = p.ids[0] | (p.ids[1] << 16);
    v.c = p.ids[2];
    v.lo = static_cast<int>(p.lo);  // <= C(m, 2) < 2^17
    v.hi = static_cast<int>(p.hi);
    v.base_lo = static_cast<int>(p.base);
    v.base_hi = static_cast<int>(p.base >> 32);
    if (alive) {
      u32 ra[8], rb[8], rc[8], s1[8], s0[8];
      scan5_load_row<STR>(s_pool, p.ids[0], ra);
      scan5_load_row<STR>(s_pool, p.ids[1], rb);
      scan5_load_row<STR>(s_pool, p.ids[2], rc);
      const Scan5ScreenCell sc = scan5_screen_cell(ra, rb, rc, T1, T0);
#pragma unroll
      for (int w = 0; w < 8; w++) {
        const u32 cell = scan5_cell_dword(ra[w], rb[w], rc[w], sc.u0);
        s1[w] = cell & T1[w];
        s0[w] = cell & T0[w];
      }
      scan5_side_head(s1, v.head1);
      scan5_side_head(s0, v.head0);
      v.cells = static_cast<int>(sc.live | (static_cast<u32>(sc.u0) << 8) |
                                 (static_cast<u32>(sc.c1) << 12) |
                                 (static_cast<u32>(sc.c0) << 21));
    }
    const u64 todo = __ballot(alive);
    if (todo == 0) continue;
    const u64 r = scan5_wave_walk<STR, ORD>(
        args, ctl, pad, (lds_cu64*)s_pool, (lds_cu32*)s_G, (lds_cu32*)s_T,
        (lds_slice*)sl, todo, v.ab, v.c, v.lo, v.hi, v.base_lo, v.base_hi,
        v.cells, v.head1[0], v.head1[1], v.head1[2], v.head1[3], v.head0[0],
        v.head0[1], v.head0[2], v.head0[3]);
    local_eval += r & ~SCAN5_WALK_STOP;
    if ((r & SCAN5_WALK_STOP) != 0) break;
  }

  block_add_evaluated(ctl, local_eval);
}

// The wave-owned variant of k_scan5<true, ORD>, for the pools where it is
// the faster one (the host chooses: SCAN5_WAVE_MIN_POOL). It walks every
// triple on the gate-transposed pool, whatever its row length.
template <bool ORD>
__global__ void __launch_bounds__(SCAN_BLOCK, 4) k_scan5_wave(
    ScanArgs args, i64 q_begin, i64 q_units) {
  scan5_wave_scan<ORD>(args, q_begin, q_units);
}

}  // namespace
}  // namespace sbg
