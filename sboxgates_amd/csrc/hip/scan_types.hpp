// scan_types.hpp — plain types and constants that the GPU scan code shares
// across translation units: the kernel modules (scan_default.hip,
// scan_ordered.hip), the persistent service (scan_service.hip) and the host
// wrapper (gpu_engine.hip). They are in namespace sbg proper, so a launcher
// can name them in its signature. Private to csrc/hip.
#pragma once

#include <hip/hip_runtime.h>

#include <cstring>
#include <stdexcept>
#include <string>

#include "sbg/scan.hpp"

// Host-side check of a HIP runtime call.
#define SBG_HIP_CHECK(expr)                                                    \
  do {                                                                         \
    hipError_t _e = (expr);                                                    \
    if (_e != hipSuccess) {                                                    \
      throw std::runtime_error(std::string("HIP error: ") +                    \
                               hipGetErrorString(_e) + " at " #expr);          \
    }                                                                          \
  } while (0)

namespace sbg {

// ---------------------------------------------------------------------------
// Device-side control block.
// ---------------------------------------------------------------------------
struct DevCtl {
  u32 abort;
  u32 lock;
  u32 found;
  u32 pool_n;  // ordered k=7: the pool size, for k_scan7_assign's ranks
  u16 res[10];
  u16 pad2[3];
  unsigned long long evaluated;
  unsigned long long queue;      // prefix dequeue counter
  unsigned long long hit_count;  // K7 filter
  u32 overflow;                  // K7 filter: hit buffer overflowed
  u32 pad3;
  // k=2: minimum over the hits of rank << 8 | matcher entry. Ordered scans
  // (ScanRequest::ordered) of the other kinds: minimum over the hits of
  // rank << 16 | function << 8 | argument order (k=3 and k=4; k=3 leaves the
  // low 16 bits zero) or of the plain rank (k=5, k=7, shared-input). The
  // host, or the service leader, sets it to all-ones before every request.
  unsigned long long best;
};

// Shift of the rank inside DevCtl::best for ordered k=3 / k=4 scans.
constexpr int BEST3_SHIFT = 16;

struct Hit7 {
  u64 p1[2];
  u64 p0[2];
  u16 nums[7];
  u16 pad;
};

// What a k=2 request carries besides the pool: the pair matcher and the
// visit order (order[j] < n for j < n; the tail is never read). Sized in
// whole u64 words so that it is copied and staged 8 bytes at a time.
struct Pair2Stage {
  u8 matcher[256];
  u16 order[(MAX_GATES + 3) / 4 * 4];
};
static_assert(sizeof(Pair2Stage) % 8 == 0);

// A k=2 request must name its matcher, and its order must stay inside the
// pool: the kernels index the LDS pool with it unchecked.
inline void check_pair2_request(const ScanRequest& rq) {
  if (rq.matcher2 == nullptr) throw std::runtime_error("scan2 needs matcher2");
  if (rq.n > MAX_GATES) throw std::runtime_error("scan2: pool too large");
  if (rq.order == nullptr) return;
  for (int j = 0; j < rq.n; j++) {
    if (rq.order[j] >= rq.n) throw std::runtime_error("scan2: order out of range");
  }
}

inline void fill_pair2_stage(Pair2Stage* out, const ScanRequest& rq) {
  std::memcpy(out->matcher, rq.matcher2->entry, sizeof(out->matcher));
  for (int j = 0; j < rq.n; j++) {
    out->order[j] = rq.order != nullptr ? rq.order[j] : static_cast<u16>(j);
  }
}

struct ScanArgs {
  const ttable* pool;  // device pool (n tables)
  DevCtl* ctl;
  Hit7* hits;          // K7 only
  u64 hit_cap;         // K7 only
  const Avail3Matcher* matcher;  // k=4 only
  const Pair2Stage* pair2;       // k=2 only
  ttable T1, T0;
  int n;
  i64 begin, end;
  u64 excl;  // excluded gate ids < 64
  u64 seed;
  int count_all;
  int slices7;  // K7: sub-quad slicing factor (dequeue unit = quad x slice)
};

constexpr int SCAN_BLOCK = 256;

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

}  // namespace sbg
