// scan_device.hpp — device-side pieces shared by the persistent k=4 / k=2
// service (scan_service.hip) and the one-shot kernel families (scan_*.hpp),
// or by at least two of those families: rank decoders, abort/publish (and,
// for ordered scans, the lowest-hit minimum that takes their place), LDS
// staging, the k=3/k=4 triple walk, the k=2 pair walk and the prefix-batch
// layer of the k=5/k=7 and shared-input scans. The plain types they work on
// (control block, kernel arguments) are in scan_types.hpp.
//
// Everything here is __device__ __forceinline__ or has internal linkage, so
// each .hip file is a self-contained translation unit (no relocatable
// device code). No i64 division in device code (it is software-emulated):
// binomials use closed forms with constant divisors (compiled to
// multiply-high).
#pragma once

#include <hip/hip_runtime.h>

#include "sbg/gpu.hpp"
#include "sbg/lutcover.hpp"
#include "sbg/rng.hpp"
#include "scan_types.hpp"

namespace sbg {
namespace {

// Closed-form binomials; constant divisors compile to multiply-high.
__device__ __forceinline__ i64 cf2(i64 x) { return x < 2 ? 0 : x * (x - 1) / 2; }
__device__ __forceinline__ i64 cf3(i64 x) {
  return x < 3 ? 0 : x * (x - 1) * (x - 2) / 6;
}
__device__ __forceinline__ i64 cf4(i64 x) {
  return x < 4 ? 0 : x * (x - 1) * (x - 2) * (x - 3) / 24;
}
__device__ __forceinline__ i64 cf5(i64 x) {
  return x < 5 ? 0 : x * (x - 1) * (x - 2) * (x - 3) * (x - 4) / 120;
}
__device__ __forceinline__ i64 cf6(i64 x) {
  return x < 6 ? 0 : x * (x - 1) * (x - 2) * (x - 3) * (x - 4) * (x - 5) / 720;
}
__device__ __forceinline__ i64 cf7(i64 x) {
  if (x < 7) return 0;
  u64 p = static_cast<u64>(x) * (x - 1) * (x - 2) * (x - 3);
  p *= static_cast<u64>(x - 4) * (x - 5) / 2;  // keep the product in range
  p *= static_cast<u64>(x - 6);
  return static_cast<i64>(p / 2520);
}
// C(x, K) for a compile-time K in [2, 7].
template <int K>
__device__ __forceinline__ i64 cf(i64 x) {
  static_assert(K >= 2 && K <= 7);
  if constexpr (K == 2) return cf2(x);
  else if constexpr (K == 3) return cf3(x);
  else if constexpr (K == 4) return cf4(x);
  else if constexpr (K == 5) return cf5(x);
  else if constexpr (K == 6) return cf6(x);
  else return cf7(x);
}

// Largest a in [0, n-k] with C(n,k) - C(n-a,k) <= r, i.e. the first element
// of the rank-r k-combination of [0,n). Binary search over a monotone
// closed form (~log2(n) probes).
template <i64 (*CF)(i64)>
__device__ __forceinline__ int first_of_rank(i64 r, int n, i64 total) {
  int lo = 0, hi = n;  // invariant: prefix(lo) <= r < prefix(hi)
  while (hi - lo > 1) {
    int mid = (lo + hi) >> 1;
    i64 prefix = total - CF(n - mid);
    if (prefix <= r) lo = mid; else hi = mid;
  }
  return lo;
}

// Flat pair index -> (d, e), 0 <= d < e < m (lexicographic d-major).
__device__ __forceinline__ void dev_decode_pair(i64 q, int m, int* d, int* e) {
  double mm = static_cast<double>(m) - 0.5;
  double disc = mm * mm - 2.0 * static_cast<double>(q) - 0.75;
  int dd = static_cast<int>(mm - 0.5 - __builtin_sqrt(disc > 0.0 ? disc : 0.0));
  if (dd < 0) dd = 0;
  if (dd > m - 2) dd = m - 2;
  // S(d) = d*m - d*(d+1)/2; fix up to the exact row.
  i64 S = static_cast<i64>(dd) * m - static_cast<i64>(dd) * (dd + 1) / 2;
  while (dd > 0 && S > q) { dd--; S -= m - 1 - dd; }
  while (S + (m - 1 - dd) <= q) { S += m - 1 - dd; dd++; }
  *d = dd;
  *e = static_cast<int>(q - S) + dd + 1;
}

// Flat triple index -> (d, e, f), 0 <= d < e < f < m.
__device__ __forceinline__ void dev_decode_triple(i64 q, int m, int* d, int* e,
                                                  int* f) {
  int dd = first_of_rank<cf3>(q, m, cf3(m));
  i64 rem = q - (cf3(m) - cf3(m - dd));
  int e2, f2;
  dev_decode_pair(rem, m - dd - 1, &e2, &f2);
  *d = dd;
  *e = dd + 1 + e2;
  *f = dd + 1 + f2;
}

// Flat rank -> the NP-combination ids[0] < ... < ids[NP-1] of [0, m),
// NP in {3, 4}.
template <int NP>
__device__ __forceinline__ void dev_decode_prefix(i64 q, int m, int* ids) {
  static_assert(NP == 3 || NP == 4);
  if constexpr (NP == 3) {
    dev_decode_triple(q, m, &ids[0], &ids[1], &ids[2]);
  } else {
    const int a = first_of_rank<cf4>(q, m, cf4(m));
    const i64 rem = q - (cf4(m) - cf4(m - a));
    dev_decode_triple(rem, m - a - 1, &ids[1], &ids[2], &ids[3]);
    ids[0] = a;
    for (int j = 1; j < 4; j++) ids[j] += a + 1;
  }
}

// Exclusion sets only cover gate ids below 64.
__device__ __forceinline__ bool dev_excluded(u64 excl, int id) {
  return id < 64 && ((excl >> id) & 1);
}

// Global-address-space pointer casts for cross-workgroup / host-visible
// words. Per the CDNA4 inter-workgroup rules (cdna_hip_programming.md
// Guideline 16): every shared word must be a GLOBAL agent/system-scope
// access — flat atomics miss the cache-bypass lowering and an XCD's
// private L2 then serves stale values to its readers forever.
typedef __attribute__((address_space(1))) unsigned svc_gu32;
typedef __attribute__((address_space(1))) unsigned long long svc_gu64;
__device__ __forceinline__ svc_gu32* as_gu32(u32* p) { return (svc_gu32*)p; }
__device__ __forceinline__ svc_gu64* as_gu64(u64* p) { return (svc_gu64*)p; }
__device__ __forceinline__ svc_gu64* as_gu64(unsigned long long* p) {
  return (svc_gu64*)p;
}

__device__ __forceinline__ bool dev_abort(const DevCtl* ctl) {
  return __hip_atomic_load(as_gu32(const_cast<u32*>(&ctl->abort)),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0;
}

// Publish a winner: single writer wins the lock; the rest skip. Payload
// (res) is plain-stored, then drained and released before the found/abort
// flag stores (Guideline 16 R1: drain -> release fence -> asm wait ->
// relaxed agent flag store), so an agent-scope reader that acquires after
// seeing found != 0 reads a complete payload on any XCD. Host readers via
// stream-sync + memcpy are ordered regardless.
__device__ __forceinline__ void dev_publish(DevCtl* ctl, const u16 res[10]) {
  if (atomicCAS(&ctl->lock, 0u, 1u) == 0u) {
    for (int i = 0; i < 10; i++) ctl->res[i] = res[i];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __hip_atomic_store(as_gu32(&ctl->found), 1u, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(as_gu32(&ctl->abort), 1u, __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
  }
}

// Ordered scans (ScanRequest::ordered): the answer is the hit of the lowest
// rank, as in walk_pairs. A hit lowers ctl->best with one relaxed agent-scope
// fetch_min on the global address; nobody takes the lock, publishes a payload
// or sets the abort flag, and no workgroup waits for another. best is only
// read to skip work that ranks above it.
__device__ __forceinline__ void dev_lower_best(DevCtl* ctl, u64 v) {
  __hip_atomic_fetch_min(as_gu64(&ctl->best), v, __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ u64 dev_best(DevCtl* ctl) {
  return __hip_atomic_load(as_gu64(&ctl->best), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
}

// ---------------------------------------------------------------------------
// Wave-level helpers of a scan whose waves run on their own (k_scan5_wave).
// ---------------------------------------------------------------------------

// A value that every lane of the wave holds alike, as a scalar.
__device__ __forceinline__ u32 dev_uniform(u32 v) {
  return static_cast<u32>(
      __builtin_amdgcn_readfirstlane(static_cast<int>(v)));
}

__device__ __forceinline__ u64 dev_uniform64(u64 v) {
  return static_cast<u64>(dev_uniform(static_cast<u32>(v))) |
         static_cast<u64>(dev_uniform(static_cast<u32>(v >> 32))) << 32;
}

// Orders a wave's LDS writes before its later LDS reads in other lanes.
// One wave's LDS operations complete in issue order, so this only has to
// keep the compiler from moving them and make it wait for the writes.
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Lane `src`'s value of v, src wave-uniform.
__device__ __forceinline__ int wave_lane_value(int v, int src) {
  return __builtin_amdgcn_readlane(v, src);
}

// dev_abort and dev_best for a whole wave, as scalars: the lanes read one
// address and branch together.
__device__ __forceinline__ bool wave_abort(const DevCtl* ctl) {
  return dev_uniform(dev_abort(ctl) ? 1u : 0u) != 0;
}
__device__ __forceinline__ u64 wave_best(DevCtl* ctl) {
  const u64 v = dev_best(ctl);
  return static_cast<u64>(dev_uniform(static_cast<u32>(v))) |
         static_cast<u64>(dev_uniform(static_cast<u32>(v >> 32))) << 32;
}

// Lexicographic rank of the ascending 7-combination ids of [0, n): the sum
// decode_prefix_window starts, carried through all seven slots.
__device__ __forceinline__ i64 dev_rank7(const u16* ids, int n) {
  i64 r = cf7(n) - cf7(n - ids[0]);
  r += cf6(n - ids[0] - 1) - cf6(n - ids[1]);
  r += cf5(n - ids[1] - 1) - cf5(n - ids[2]);
  r += cf4(n - ids[2] - 1) - cf4(n - ids[3]);
  r += cf3(n - ids[3] - 1) - cf3(n - ids[4]);
  r += cf2(n - ids[4] - 1) - cf2(n - ids[5]);
  return r + (ids[6] - ids[5] - 1);
}

// LDS pool stride: 6 u64 (48 B) per gate instead of 4 (32 B). A 32 B
// stride puts ds_read_b128 lane groups on 8-way-conflicting banks when
// lanes read consecutive gate ids; 48 B (12 dwords, 16 B aligned) spreads
// a 16-lane group over 16 distinct banks (measured: SQ_LDS_BANK_CONFLICT
// was 21% of LDS cycles at stride 32).
constexpr int PSTR = 6;

// Dense stride, 4 u64 (32 B) per gate: for a kernel whose hot loop does not
// read pool rows per candidate and that needs the LDS for something else
// (k_scan5's wide path, which keeps the gate-transposed pool next to it).
constexpr int PSTR_DENSE = 4;

template <int STR = PSTR>
__device__ __forceinline__ void load_pool_lds(u64* s_pool, const ttable* pool,
                                              int n) {
  const u64* src = reinterpret_cast<const u64*>(pool);
  for (int i = threadIdx.x; i < n * 4; i += blockDim.x) {
    s_pool[(i >> 2) * STR + (i & 3)] = src[i];
  }
}

// Stage the k=4 function matcher: bitmap, function list and count.
constexpr int MATCHER_BITMAP_BYTES = 256 * 256 / 8;
__device__ __forceinline__ void load_matcher_lds(u8* s_bitmap, u8* s_funs,
                                                 int* s_count,
                                                 const Avail3Matcher* matcher) {
  for (int i = threadIdx.x; i < MATCHER_BITMAP_BYTES / 8; i += blockDim.x) {
    reinterpret_cast<u64*>(s_bitmap)[i] =
        reinterpret_cast<const u64*>(matcher->bitmap)[i];
  }
  for (int i = threadIdx.x; i < 256 / 8; i += blockDim.x) {
    reinterpret_cast<u64*>(s_funs)[i] =
        reinterpret_cast<const u64*>(matcher->funs)[i];
  }
  if (threadIdx.x == 0) *s_count = matcher->count;
}

// Sum of every thread's evaluated count over the workgroup, returned to
// all threads. Contains barriers: call it from uniform control flow.
__device__ __forceinline__ unsigned long long block_sum_evaluated(
    u64 local_eval) {
  __shared__ unsigned long long s_eval;
  if (threadIdx.x == 0) s_eval = 0;
  __syncthreads();
  atomicAdd(&s_eval, static_cast<unsigned long long>(local_eval));
  __syncthreads();
  return s_eval;
}

// Per-block evaluated reduction: one global atomic per workgroup.
__device__ __forceinline__ void block_add_evaluated(DevCtl* ctl,
                                                    u64 local_eval) {
  const unsigned long long sum = block_sum_evaluated(local_eval);
  if (threadIdx.x == 0) atomicAdd(&ctl->evaluated, sum);
}

// ---------------------------------------------------------------------------
// Triple walk shared by the 3-LUT scan, the one-shot k=4 kernel and the
// persistent k=4 service: grid-strided walk of triple ranks [idx0, end)
// with stride `stride`, pool staged in LDS by the caller. Every triple
// whose p-masks are consistent goes to on_feasible(idx, a, b, c, p1, p0);
// a true return ends this thread's walk. Returns this thread's evaluated
// count. ORD (ordered scan): the poll leaves once the thread's own rank,
// which only grows, is past the best known (rank << BEST3_SHIFT in
// ctl->best), instead of reading the abort flag.
// ---------------------------------------------------------------------------
template <bool ORD = false, class OnFeasible>
__device__ __forceinline__ u64 walk_triples(const u64* s_pool, int n,
                                            const ttable& T1, const ttable& T0,
                                            int count_all, DevCtl* ctl,
                                            i64 idx0, i64 end, i64 stride,
                                            OnFeasible on_feasible) {
  u64 local_eval = 0;
  int tick = 0;
  for (i64 idx = idx0; idx < end; idx += stride) {
    if (((tick++) & 255) == 0 && !count_all) {
      if constexpr (ORD) {
        if (static_cast<u64>(idx) > (dev_best(ctl) >> BEST3_SHIFT)) break;
      } else {
        if (dev_abort(ctl)) break;
      }
    }
    int a, b, c;
    dev_decode_triple(idx, n, &a, &b, &c);

    local_eval++;
    // Copy out of LDS: the padded 48 B stride is not ttable-aligned, so a
    // reinterpret_cast would be UB.
    ttable ta, tb, tc;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      ta.w[w] = s_pool[a * PSTR + w];
      tb.w[w] = s_pool[b * PSTR + w];
      tc.w[w] = s_pool[c * PSTR + w];
    }
    u32 p1, p0;
    if (!lut3_p_masks(ta, tb, tc, T1, T0, &p1, &p0)) continue;
    if (on_feasible(idx, a, b, c, p1, p0)) break;
  }
  return local_eval;
}

// Cooperative copy of a k=2 stage, global to global or into LDS.
__device__ __forceinline__ void copy_pair2_stage(Pair2Stage* dst,
                                                const Pair2Stage* src) {
  for (int i = threadIdx.x; i < static_cast<int>(sizeof(Pair2Stage) / 8);
       i += blockDim.x) {
    reinterpret_cast<u64*>(dst)[i] = reinterpret_cast<const u64*>(src)[i];
  }
}

// ---------------------------------------------------------------------------
// Pair walk shared by the one-shot k=2 kernel and the persistent service:
// grid-strided walk of pair ranks [idx0, end) with stride `stride` over
// visit positions i < k, pool and Pair2Stage staged in LDS by the caller.
// The scan's answer is the hit of the lowest rank, so a hit only lowers
// ctl->best (rank << 8 | matcher entry) and nobody is told to stop: a
// thread leaves once its own rank, which only grows, is past the best
// known. No lock, no publish, no abort flag.
// ---------------------------------------------------------------------------
__device__ __forceinline__ void walk_pairs(const u64* s_pool,
                                           const Pair2Stage* s_pair2, int n,
                                           const ttable& T1, const ttable& T0,
                                           DevCtl* ctl, i64 idx0, i64 end,
                                           i64 stride) {
  if (n < 2) return;
  if (end > cf2(n)) end = cf2(n);
  int tick = 0;
  for (i64 idx = idx0; idx < end; idx += stride) {
    if (((tick++) & 255) == 0) {
      const u64 best = __hip_atomic_load(as_gu64(&ctl->best), __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT);
      if (static_cast<u64>(idx) > (best >> 8)) break;
    }
    int i, k;
    dev_decode_pair(idx, n, &i, &k);
    const int x = s_pair2->order[i], y = s_pair2->order[k];
    // Per cell p = vx << 1 | vy: the target-1 and the target-0 content.
    u64 c1[4] = {0, 0, 0, 0}, c0[4] = {0, 0, 0, 0};
#pragma unroll
    for (int w = 0; w < 4; w++) {
      const u64 tx = s_pool[x * PSTR + w], ty = s_pool[y * PSTR + w];
      const u64 x1 = tx & T1.w[w], n1 = T1.w[w] ^ x1;
      const u64 x0 = tx & T0.w[w], n0 = T0.w[w] ^ x0;
      const u64 a = x1 & ty, b = n1 & ty, c = x0 & ty, d = n0 & ty;
      c1[3] |= a;
      c1[2] |= x1 ^ a;
      c1[1] |= b;
      c1[0] |= n1 ^ b;
      c0[3] |= c;
      c0[2] |= x0 ^ c;
      c0[1] |= d;
      c0[0] |= n0 ^ d;
    }
    u32 r1 = 0, r0 = 0;
#pragma unroll
    for (int p = 0; p < 4; p++) {
      r1 |= static_cast<u32>(c1[p] != 0) << p;
      r0 |= static_cast<u32>(c0[p] != 0) << p;
    }
    if ((r1 & r0) != 0) continue;  // a cell forced both ways
    const u32 e = s_pair2->matcher[(r1 | r0) << 4 | r1];
    if (e == PAIR2_NONE) continue;
    __hip_atomic_fetch_min(as_gu64(&ctl->best), static_cast<u64>(idx) << 8 | e,
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    break;  // this thread's later ranks are all higher
  }
}

// ---------------------------------------------------------------------------
// K1c — gate-mode step-4 triple scan: triples realized by an available
// composed 3-input function in one of 6 argument orders. The per-candidate
// function search is one bitmap probe per order (matcher precomputed on the
// host), replacing the reference's 256-function x 4-order truth-table loop
// (sboxgates.c:392-435).
// ---------------------------------------------------------------------------
__device__ __forceinline__ u8 dev_permute_cells8(u8 m, int s0, int s1, int s2) {
  u8 out = 0;
#pragma unroll
  for (int c = 0; c < 8; c++) {
    if (!((m >> c) & 1)) continue;
    int v[3] = {(c >> 2) & 1, (c >> 1) & 1, c & 1};
    out |= static_cast<u8>(1u << ((v[s0] << 2) | (v[s1] << 1) | v[s2]));
  }
  return out;
}

__constant__ int c_perm6[6][3] = {{0, 1, 2}, {0, 2, 1}, {1, 0, 2},
                                  {1, 2, 0}, {2, 0, 1}, {2, 1, 0}};

// The k=4 action for walk_triples, matcher staged in LDS by the caller.
// Used by both the one-shot k_scan4 kernel and the persistent service.
// ORD (ordered scan): a hit lowers ctl->best with rank << BEST3_SHIFT |
// function index << 8 | argument order and ends the thread's walk, whose
// later ranks are all higher; the first order, then the first function, are
// cpu_scan4's.
template <bool ORD = false>
struct Scan4Match {
  const u8* s_bitmap;
  const u8* s_funs;
  int s_count;
  int count_all;
  DevCtl* ctl;

  __device__ __forceinline__ bool operator()(i64 idx, int a, int b, int c,
                                             u32 p1, u32 p0) const {
    if (count_all) return false;
    const u8 req1 = static_cast<u8>(p1);
    const u8 care = static_cast<u8>(p1 | p0);
    for (int perm = 0; perm < 6; perm++) {
      const u8 r = dev_permute_cells8(req1, c_perm6[perm][0], c_perm6[perm][1],
                                      c_perm6[perm][2]);
      const u8 cr = dev_permute_cells8(care, c_perm6[perm][0], c_perm6[perm][1],
                                       c_perm6[perm][2]);
      const int bidx = cr * 256 + r;
      if (!((s_bitmap[bidx >> 3] >> (bidx & 7)) & 1)) continue;
      for (int f = 0; f < s_count; f++) {
        if ((s_funs[f] & cr) == r) {
          if constexpr (ORD) {
            dev_lower_best(ctl, static_cast<u64>(idx) << BEST3_SHIFT |
                                    static_cast<u64>(f) << 8 |
                                    static_cast<u64>(perm));
            return true;
          }
          u16 res[10] = {};
          res[0] = static_cast<u16>(f);
          res[1] = static_cast<u16>(perm);
          res[2] = static_cast<u16>(a);
          res[3] = static_cast<u16>(b);
          res[4] = static_cast<u16>(c);
          dev_publish(ctl, res);
          break;
        }
      }
      break;  // bitmap said a function exists; it was found and published
    }
    if constexpr (ORD) return false;
    return dev_abort(ctl);
  }
};

// ---------------------------------------------------------------------------
// Prefix-batch layer of the k=5 (NP = 3), k=7 (NP = 4) and shared-input
// (NP = 3 of K = 4) scans. A
// workgroup dequeues a batch of NB prefix units; NB threads decode one
// prefix each and clip its tail window to the scan range; the 2^NP prefix
// cells, masked with target-1 / target-0, are built cooperatively into LDS
// and the cells that can contradict are marked live.
// ---------------------------------------------------------------------------

// One dequeue per batch: thread 0 takes `units` off ctl->queue and
// broadcasts the first one through *s_slot. Returns -1 instead when the
// scan was aborted (or, if watched, the K7 hit buffer overflowed).
// Contains barriers. ORD (ordered scan): a known hit takes the abort flag's
// place. The queue hands out prefixes in increasing order, so every prefix
// not yet dequeued ranks above any hit already known.
template <bool ORD = false>
__device__ __forceinline__ i64 dequeue_batch(DevCtl* ctl, int units,
                                             int count_all, bool watch_overflow,
                                             i64* s_slot) {
  __syncthreads();
  if (threadIdx.x == 0) {
    const bool halt =
        (!count_all && (ORD ? dev_best(ctl) != ~0ULL : dev_abort(ctl))) ||
        (watch_overflow &&
         __hip_atomic_load(&ctl->overflow, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT) != 0);
    *s_slot = halt ? -1
                   : static_cast<i64>(__hip_atomic_fetch_add(
                         &ctl->queue, static_cast<unsigned long long>(units),
                         __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  }
  __syncthreads();
  const i64 batch_base = *s_slot;
  __syncthreads();
  return batch_base;
}

// One NP-prefix of a K-combination scan over a pool of n gates (K = 2 NP - 1
// for the k=5 and k=7 scans, K = 4 with NP = 3 for the shared-input scan):
// its gate ids, the flat rank `base` of its first combination, the number m
// of gates behind its last id, and the window [lo, hi) of its C(m, K - NP)
// tail combinations that lies inside [begin, end). base < 0: no prefix.
template <int NP>
struct PrefixWindow {
  int ids[NP] = {};
  int m = 0;
  i64 base = -1, lo = 0, hi = 0;
};

template <int NP, int K = 2 * NP - 1>
__device__ __forceinline__ PrefixWindow<NP> decode_prefix_window(
    i64 pidx, i64 total, const ScanArgs& args) {
  static_assert(K > NP && K - 2 >= 2);
  PrefixWindow<NP> p;
  if (pidx >= total) return p;
  const int n = args.n;
  dev_decode_prefix<NP>(pidx, n, p.ids);
  // base = sum_j C(n - ids[j-1] - 1, K - j) - C(n - ids[j], K - j).
  p.base = cf<K>(n) - cf<K>(n - p.ids[0]);
  p.base += cf<K - 1>(n - p.ids[0] - 1) - cf<K - 1>(n - p.ids[1]);
  p.base += cf<K - 2>(n - p.ids[1] - 1) - cf<K - 2>(n - p.ids[2]);
  if constexpr (NP == 4) {
    p.base += cf<K - 3>(n - p.ids[2] - 1) - cf<K - 3>(n - p.ids[3]);
  }
  p.m = n - 1 - p.ids[NP - 1];
  i64 ntail;
  if constexpr (K - NP == 1) ntail = p.m; else ntail = cf<K - NP>(p.m);
  p.lo = args.begin > p.base ? args.begin - p.base : 0;
  p.hi = args.end - p.base < ntail ? args.end - p.base : ntail;
  return p;
}

// Empty the window of a prefix that lies past the range, has nothing left
// in it, or holds an excluded gate.
template <int NP>
__device__ __forceinline__ void drop_dead_prefix(PrefixWindow<NP>& p,
                                                 const ScanArgs& args) {
  if (p.base < 0) return;
  bool excl_prefix = false;
  if (args.excl != 0) {
    for (int j = 0; j < NP; j++) {
      excl_prefix = excl_prefix || dev_excluded(args.excl, p.ids[j]);
    }
  }
  if (p.base >= args.end || p.lo >= p.hi || excl_prefix) p.lo = p.hi = 0;
}

// Cooperative prefix-cell build: NB x 2^NP cells x 4 words x {1,0} items
// (512 for the k=5 and k=7 scans, two per thread). s_prefix holds the prefix
// sums of the window sizes; empty windows are skipped.
template <int NP, int NB, int STR = PSTR>
__device__ __forceinline__ void build_prefix_cells(
    const u64* s_pool, const u16 (*s_ids)[NP], const i64* s_prefix,
    const ttable& T1, const ttable& T0, u64 (*s_H1)[1 << NP][4],
    u64 (*s_H0)[1 << NP][4]) {
  constexpr int CELLS = 1 << NP;
  constexpr int half = NB * CELLS * 4;
  for (int item = threadIdx.x; item < 2 * half; item += blockDim.x) {
    const bool is1 = item < half;
    const int it = is1 ? item : item - half;
    const int t = it / (CELLS * 4);
    const int u = (it >> 2) & (CELLS - 1);
    const int w = it & 3;
    if (s_prefix[t + 1] == s_prefix[t]) continue;
    u64 cell = ~0ULL;
#pragma unroll
    for (int j = 0; j < NP; j++) {
      const u64 row = s_pool[s_ids[t][j] * STR + w];
      cell &= ((u >> (NP - 1 - j)) & 1) ? row : ~row;
    }
    if (is1) {
      s_H1[t][u][w] = cell & T1.w[w];
    } else {
      s_H0[t][u][w] = cell & T0.w[w];
    }
  }
}

// Liveness: a cell whose H1 or H0 side is empty can never contradict
// (and survivors rebuild exact p-masks anyway). Sparse-mask scans in
// deep recursion typically keep only a few of the 2^NP cells live.
// Thread i < NB * 2^NP tests cell (i >> NP, i & (2^NP - 1)), sets its bit
// in s_live and returns true if it is live. Contains a barrier after the
// s_live reset; the caller places the one that publishes s_live.
template <int NP, int NB>
__device__ __forceinline__ bool mark_live_cells(const u64 (*s_H1)[1 << NP][4],
                                                const u64 (*s_H0)[1 << NP][4],
                                                u32* s_live) {
  constexpr int CELLS = 1 << NP;
  if (threadIdx.x < NB) s_live[threadIdx.x] = 0;
  __syncthreads();
  if (threadIdx.x >= NB * CELLS) return false;
  const int t = threadIdx.x >> NP;
  const int u = threadIdx.x & (CELLS - 1);
  const u64 h1 = s_H1[t][u][0] | s_H1[t][u][1] | s_H1[t][u][2] | s_H1[t][u][3];
  const u64 h0 = s_H0[t][u][0] | s_H0[t][u][1] | s_H0[t][u][2] | s_H0[t][u][3];
  if (h1 == 0 || h0 == 0) return false;
  atomicOr(&s_live[t], 1u << u);
  return true;
}

}  // namespace
}  // namespace sbg
