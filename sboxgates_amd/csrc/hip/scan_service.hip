// scan_service.hip — persistent scan service: the resident k_scan4_service
// kernel (k=4 triple scans and k=2 pair scans), its mailbox protocol and
// the host ScanService.
//
// Gate-mode searches issue one step-4 triple scan per recursion node
// (~600k nodes for AES bit 0); through the one-shot launch path each scan
// pays a ~30 us API floor (pool H2D + ctl round trips + launch + sync) that
// dwarfs the kernel time of small scans. The service keeps a grid of
// resident workgroups parked on a mailbox in fine-grained pinned host
// memory: the host publishes {request header, pool delta} with one release
// store, workgroup 0 copies the delta into the device pool and re-publishes
// device-side, and the last workgroup to finish writes the response
// directly back to pinned memory — no launches, no stream ops, ~5-8 us per
// scan. (Price anchors: MI355X_MICROARCH.md persistent-kernel price list —
// host-paired flag round trips are single-digit us; relaxed polls +
// s_sleep from one lane, one acquire fence on the hit.)
//
// Liveness/safety design (every wait is bounded):
//  * The kernel retires itself after ~2 ms idle (svc_state -> RETIRED) so
//    an idle service never starves other kernels of CUs; the host reaps
//    and relaunches on the next submit (and resolves the publish/retire
//    race by relaunching when it observes RETIRED while waiting).
//  * Residency self-check: workgroups count themselves in at startup; if
//    the grid is not fully resident within a deadline the host quits the
//    kernel and permanently falls back to the one-shot path.
//  * The host can always stop the kernel without its cooperation: leader
//    workgroup polls quit_req (host memory); the other workgroups poll
//    dev_seq (device memory) which the host can overwrite via an async
//    copy on a separate stream, and the scan loops poll ctl.abort which
//    the host can set the same way.

#include "scan_service.hpp"

#include <algorithm>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <thread>

#include "scan_device.hpp"

namespace sbg {

enum : u32 { SVC_RUNNING = 1u, SVC_RETIRED = 2u };

// Request header word layout (u64[16] block, read cooperatively).
enum {
  HDR_N_KEEP = 0,     // n (lo32) | pool_keep (hi32)
  HDR_EPOCH_CALL = 1, // matcher_epoch (lo32) | count_all (hi32)
  HDR_BEGIN = 2,
  HDR_END = 3,
  HDR_OP = 4,         // scan kind: 4 (triples) or 2 (pairs)
  HDR_ORDERED = 5,    // k=4: nonzero for an ordered scan (lowest hit rank)
                      // 6..7 reserved
  HDR_T1 = 8,         // 8..11
  HDR_T0 = 12,        // 12..15
  HDR_WORDS = 16,
};

struct SvcMailbox {  // pinned fine-grained host memory
  // host -> device control
  u64 req_seq;       // release-stored by the host to publish a request
  u32 quit_req;
  u32 svc_state;     // SVC_RUNNING / SVC_RETIRED
  // device -> host
  u64 resp_seq;      // flag-stored by the last workgroup (after a drain)
  u64 r_evaluated;
  u32 r_found;
  u32 alive;         // residency self-check counter
  u64 r_res_w[3];    // res[10] packed 4 x u16 per word
  // request payload
  alignas(64) u64 hdr[HDR_WORDS];
  alignas(64) ttable pool_staging[MAX_GATES];  // full pool image (host shadow)
  alignas(64) Avail3Matcher matcher_staging;
  alignas(64) Pair2Stage pair2_staging;  // k=2: rewritten by every request
};

struct SvcDev {  // device memory
  u64 dev_seq;   // published seq for non-leader workgroups
  u32 matcher_epoch;
  unsigned long long done;
  DevCtl ctl;
  alignas(64) u64 hdr[HDR_WORDS];
  alignas(64) ttable pool[MAX_GATES];
  alignas(64) Avail3Matcher matcher;
  alignas(64) Pair2Stage pair2;
};

namespace {

// Leader poll iterations before idle retirement (each ~1-2 us: one PCIe
// read + s_sleep) — about a second. Gate-mode searches interleave CPU
// scans between service requests, so a short timeout causes relaunch
// storms; in-process k=5/7 launches park the service explicitly instead.
inline int svc_idle_polls() {
  static const int v = [] {
    const char* s = std::getenv("SBOXGATES_SVC_IDLE");
    return s != nullptr ? std::atoi(s) : 500000;
  }();
  return v;
}

__global__ void __launch_bounds__(SCAN_BLOCK) k_scan4_service(SvcMailbox* mb,
                                                              SvcDev* dev,
                                                              int c_idle_polls,
                                                              u64 served0) {
  __shared__ alignas(16) u64 s_pool[MAX_GATES * PSTR];
  __shared__ alignas(16) u8 s_bitmap[MATCHER_BITMAP_BYTES];
  __shared__ u8 s_funs[256];
  // A k=2 request has no use for the k=4 bitmap, which every k=4 request
  // stages afresh: its matcher and order take the bitmap's place.
  static_assert(sizeof(Pair2Stage) <= MATCHER_BITMAP_BYTES);
  Pair2Stage* s_pair2 = reinterpret_cast<Pair2Stage*>(s_bitmap);
  __shared__ alignas(16) u64 s_hdr[HDR_WORDS];
  __shared__ u64 s_word;
  __shared__ int s_count;

  if (threadIdx.x == 0) {
    __hip_atomic_fetch_add(as_gu32(&mb->alive), 1u, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
  }

  const bool leader = blockIdx.x == 0;
  // Protocol word: (req_seq << 1) | quit. Monotonic; one word carries both
  // the sequence and the command, so publish/consume is a single-flag
  // hand-off (Guideline 16 R2 style). A fresh kernel starts from the word
  // of the last request the host has an answer to (dev_seq starts there
  // too), so it does not take that request for a new one: the host does not
  // wait for such a replay, and a leader that went on to the next request
  // while other workgroups were still in the replay reset the counters
  // under them (a response before the scan was done, or counts of both).
  u64 served = served0;

  for (;;) {
    // ---- wait for a request (or quit) ----
    if (threadIdx.x == 0) {
      u64 word;
      if (leader) {
        int idle = 0;
        for (;;) {
          u64 rs = __hip_atomic_load(as_gu64(&mb->req_seq), __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_SYSTEM);
          if ((rs << 1) != served) {
            word = rs << 1;
            break;
          }
          if (__hip_atomic_load(as_gu32(&mb->quit_req), __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_SYSTEM) != 0) {
            word = served + 3;  // bump seq, set quit bit
            break;
          }
          if (++idle > c_idle_polls) {
            // Retire. After this store the kernel never touches the
            // mailbox again; the host reaps and relaunches on demand.
            __hip_atomic_store(as_gu32(&mb->svc_state), SVC_RETIRED,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            word = served + 3;
            break;
          }
          __builtin_amdgcn_s_sleep(32);
        }
      } else {
        for (;;) {
          u64 ds = __hip_atomic_load(as_gu64(&dev->dev_seq), __ATOMIC_RELAXED,
                                     __HIP_MEMORY_SCOPE_AGENT);
          if (ds != served) {
            word = ds;
            break;
          }
          __builtin_amdgcn_s_sleep(16);
        }
      }
      // ONE acquire after the poll match (covers the workgroup: a
      // __syncthreads() follows). System scope: the leader's payload
      // source is host memory.
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "");
      s_word = word;
    }
    __syncthreads();
    const u64 word = s_word;
    const bool quit = (word & 1) != 0;
    const u64 seq = word >> 1;

    if (leader) {
      if (!quit) {
        // Pull the request: header block, pool delta, matcher delta.
        if (threadIdx.x < HDR_WORDS) s_hdr[threadIdx.x] = mb->hdr[threadIdx.x];
        __syncthreads();
        // Defensive clamps: a corrupt header must never walk past the
        // fixed-size pool buffers (a GPU page fault can wedge the node).
        const int n = std::min(
            static_cast<int>(s_hdr[HDR_N_KEEP] & 0xFFFFFFFFu), MAX_GATES);
        const int keep = std::max(
            0, std::min(static_cast<int>(s_hdr[HDR_N_KEEP] >> 32), n));
        const u32 epoch = static_cast<u32>(s_hdr[HDR_EPOCH_CALL] & 0xFFFFFFFFu);
        if (threadIdx.x < HDR_WORDS) dev->hdr[threadIdx.x] = s_hdr[threadIdx.x];
        {
          const u64* src = reinterpret_cast<const u64*>(mb->pool_staging);
          u64* dst = reinterpret_cast<u64*>(dev->pool);
          for (int i = keep * 4 + threadIdx.x; i < n * 4; i += blockDim.x) {
            dst[i] = src[i];
          }
        }
        if (epoch != dev->matcher_epoch) {
          const u64* ms = reinterpret_cast<const u64*>(&mb->matcher_staging);
          u64* md = reinterpret_cast<u64*>(&dev->matcher);
          // Round UP: sizeof(Avail3Matcher) is not a multiple of 8 and the
          // last partial word holds `count`; truncating it left s_count = 0
          // and made every early-exit probe silently miss. Both structs sit
          // in 64-aligned tails, so the overread is in-allocation padding.
          for (size_t i = threadIdx.x; i < (sizeof(Avail3Matcher) + 7) / 8;
               i += blockDim.x) {
            md[i] = ms[i];
          }
          __syncthreads();
          if (threadIdx.x == 0) dev->matcher_epoch = epoch;
        }
        if (s_hdr[HDR_OP] == 2) {
          copy_pair2_stage(&dev->pair2, &mb->pair2_staging);
        }
        if (threadIdx.x == 0) {
          dev->done = 0;
          dev->ctl.best = ~0ULL;
          dev->ctl.abort = 0;
          dev->ctl.lock = 0;
          dev->ctl.found = 0;
          dev->ctl.evaluated = 0;
          dev->ctl.queue = 0;
          dev->ctl.hit_count = 0;
          dev->ctl.overflow = 0;
        }
      }
      // Publish to the other workgroups (Guideline 16 counter form):
      // every wave drains its plain stores, then one lane releases and
      // stores the flag word relaxed.
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(as_gu64(&dev->dev_seq), word, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      }
      __syncthreads();
    }
    if (quit) return;
    served = word;

    // ---- stage request + pool + matcher into LDS ----
    if (!leader) {
      if (threadIdx.x < HDR_WORDS) s_hdr[threadIdx.x] = dev->hdr[threadIdx.x];
    }
    __syncthreads();
    const int n = std::min(static_cast<int>(s_hdr[HDR_N_KEEP] & 0xFFFFFFFFu),
                           MAX_GATES);
    const int count_all = static_cast<int>(s_hdr[HDR_EPOCH_CALL] >> 32);
    const i64 begin = static_cast<i64>(s_hdr[HDR_BEGIN]);
    const i64 end = static_cast<i64>(s_hdr[HDR_END]);
    ttable T1, T0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      T1.w[w] = s_hdr[HDR_T1 + w];
      T0.w[w] = s_hdr[HDR_T0 + w];
    }
    const bool pairs = s_hdr[HDR_OP] == 2;
    const bool ordered = !pairs && s_hdr[HDR_ORDERED] != 0;
    load_pool_lds(s_pool, dev->pool, n);
    if (pairs) {
      copy_pair2_stage(s_pair2, &dev->pair2);
    } else {
      load_matcher_lds(s_bitmap, s_funs, &s_count, &dev->matcher);
    }
    __syncthreads();

    // ---- scan ----
    const i64 stride = static_cast<i64>(gridDim.x) * blockDim.x;
    const i64 idx0 =
        begin + blockIdx.x * static_cast<i64>(blockDim.x) + threadIdx.x;
    u64 local_eval = 0;
    if (pairs) {
      walk_pairs(s_pool, s_pair2, n, T1, T0, &dev->ctl, idx0, end, stride);
      // Every wave's fetch_min has landed before the barriers below let
      // thread 0 take its ticket.
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else if (ordered) {
      local_eval = walk_triples<true>(
          s_pool, n, T1, T0, count_all, &dev->ctl, idx0, end, stride,
          Scan4Match<true>{s_bitmap, s_funs, s_count, count_all, &dev->ctl});
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // as for pairs
    } else {
      local_eval = walk_triples<false>(
          s_pool, n, T1, T0, count_all, &dev->ctl, idx0, end, stride,
          Scan4Match<false>{s_bitmap, s_funs, s_count, count_all, &dev->ctl});
    }

    // ---- completion: last workgroup publishes the response ----
    // The shared reduction zeroes its LDS word itself: one more workgroup
    // barrier per request, ahead of the sequence below, whose order stays.
    const unsigned long long block_eval = block_sum_evaluated(local_eval);
    if (threadIdx.x == 0) {
      if (block_eval != 0) {
        __hip_atomic_fetch_add(as_gu64(&dev->ctl.evaluated), block_eval,
                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
      // Fence-then-ticket order (Guideline 16 split-K recipe).
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      unsigned long long d = __hip_atomic_fetch_add(
          as_gu64(&dev->done), 1ULL, __ATOMIC_RELAXED,
          __HIP_MEMORY_SCOPE_AGENT);
      if (d == gridDim.x - 1ULL) {
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        unsigned long long ev = __hip_atomic_load(
            as_gu64(&dev->ctl.evaluated), __ATOMIC_RELAXED,
            __HIP_MEMORY_SCOPE_AGENT);
        u32 found = __hip_atomic_load(as_gu32(&dev->ctl.found),
                                      __ATOMIC_RELAXED,
                                      __HIP_MEMORY_SCOPE_AGENT);
        u64 rw[3] = {0, 0, 0};
        if (pairs) {
          // The answer is the minimum: decode it into the response words
          // (layout: cpu_scan2).
          const i64 total = cf2(n);
          const i64 e2 = end < total ? end : total;
          const unsigned long long best = __hip_atomic_load(
              as_gu64(&dev->ctl.best), __ATOMIC_RELAXED,
              __HIP_MEMORY_SCOPE_AGENT);
          const i64 rank = static_cast<i64>(best >> 8);
          found = best != ~0ULL && n >= 2 && rank >= begin && rank < e2;
          ev = e2 > begin ? static_cast<unsigned long long>(e2 - begin) : 0;
          if (found != 0) {
            int i, k;
            dev_decode_pair(rank, n, &i, &k);
            const u64 x = s_pair2->order[i], y = s_pair2->order[k];
            const bool swapped = (best & 0x80) != 0;
            rw[0] = (best & 0x7F) | (swapped ? 1ULL << 16 : 0) |
                    (swapped ? y : x) << 32 | (swapped ? x : y) << 48;
            ev = static_cast<unsigned long long>(rank - begin + 1);
          }
        } else if (ordered) {
          // Likewise (layout: cpu_scan4). The walk only visits ranks of the
          // window, so a hit lies inside it.
          const unsigned long long best = __hip_atomic_load(
              as_gu64(&dev->ctl.best), __ATOMIC_RELAXED,
              __HIP_MEMORY_SCOPE_AGENT);
          found = best != ~0ULL;
          if (found != 0) {
            int a, b, c;
            dev_decode_triple(static_cast<i64>(best >> BEST3_SHIFT), n, &a, &b,
                              &c);
            rw[0] = ((best >> 8) & 0xFF) | (best & 0xFF) << 16 |
                    static_cast<u64>(a) << 32 | static_cast<u64>(b) << 48;
            rw[1] = static_cast<u64>(c);
          }
        } else if (found != 0) {
          for (int i = 0; i < 10; i++) {
            rw[i >> 2] |= static_cast<u64>(dev->ctl.res[i]) << ((i & 3) * 16);
          }
        }
        // Response: relaxed system stores (write-through), drained before
        // the resp_seq flag store.
        __hip_atomic_store(as_gu64(&mb->r_evaluated), ev, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
        __hip_atomic_store(as_gu32(&mb->r_found), found, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
        for (int i = 0; i < 3; i++) {
          __hip_atomic_store(as_gu64(&mb->r_res_w[i]), rw[i], __ATOMIC_RELAXED,
                             __HIP_MEMORY_SCOPE_SYSTEM);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_store(as_gu64(&mb->resp_seq), seq, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_SYSTEM);
      }
    }
  }
}

std::mutex g_svc_mu;
std::map<int, std::weak_ptr<ScanService>> g_svc_registry;

// Size of the SvcDev control header (everything the host must reset before
// a relaunch; pool/matcher content survives, matcher_epoch reset forces a
// re-copy).
constexpr size_t SVC_DEV_CTL_BYTES = offsetof(SvcDev, hdr);
static_assert(offsetof(SvcDev, dev_seq) == 0 &&
              offsetof(SvcDev, matcher_epoch) < offsetof(SvcDev, ctl) &&
              offsetof(SvcDev, done) < offsetof(SvcDev, ctl) &&
              offsetof(SvcDev, ctl) + sizeof(DevCtl) <= SVC_DEV_CTL_BYTES);

}  // namespace

static bool svc_debug() {
  static const bool on = [] {
    const char* s = std::getenv("SBOXGATES_SVC_DEBUG");
    return s != nullptr && s[0] != '\0' && s[0] != '0';
  }();
  return on;
}

ScanService::ScanService(int device) : device_(device) {
  SBG_HIP_CHECK(hipSetDevice(device_));
  SBG_HIP_CHECK(hipStreamCreate(&stream_));
  SBG_HIP_CHECK(hipStreamCreate(&esc_stream_));
  SBG_HIP_CHECK(hipHostMalloc(&mb_, sizeof(SvcMailbox), hipHostMallocCoherent));
  std::memset(mb_, 0, sizeof(SvcMailbox));
  SBG_HIP_CHECK(hipMalloc(&d_svc_, sizeof(SvcDev)));
  SBG_HIP_CHECK(hipMemset(d_svc_, 0, sizeof(SvcDev)));
  int per_cu = 0;
  SBG_HIP_CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(
      &per_cu, reinterpret_cast<const void*>(k_scan4_service), SCAN_BLOCK, 0));
  hipDeviceProp_t prop;
  SBG_HIP_CHECK(hipGetDeviceProperties(&prop, device_));
  // Small grid by design: the scans the service exists for are <= ~3e5
  // candidates (deep-recursion step-4 scans), and the request/response
  // round trip scales with the completion barrier — the flat-counter
  // barrier price is ~7-26 us at 256-1024 workgroups
  // (MI355X_MICROARCH.md barrier-counter) but single-digit at 128. A
  // 128-WG grid also coexists with other kernels (half the CUs stay
  // empty), so an idle-resident service cannot starve them.
  grid_ = std::clamp(std::min(per_cu * prop.multiProcessorCount, 64), 8, 2048);
  if (const char* g = std::getenv("SBOXGATES_SVC_GRID")) {
    long v = std::strtol(g, nullptr, 10);
    if (v >= 1 && v <= 4096) grid_ = static_cast<int>(v);
  }
  if (svc_debug()) {
    std::fprintf(stderr, "[svc] device %d: occupancy %d/CU x %d CUs -> grid %d\n",
                 device_, per_cu, prop.multiProcessorCount, grid_);
  }
}

ScanService::~ScanService() {
  std::lock_guard<std::mutex> lk(mu_);
  bool freed_ok = true;
  if (running_) {
    (void)hipSetDevice(device_);
    freed_ok = quit_bounded();
    if (!freed_ok) {
      std::fprintf(stderr,
                   "sboxgates: scan service kernel did not exit; leaking its "
                   "resources\n");
    }
  }
  if (freed_ok) {
    if (d_svc_ != nullptr) (void)hipFree(d_svc_);
    if (mb_ != nullptr) (void)hipHostFree(mb_);
    if (stream_ != nullptr) (void)hipStreamDestroy(stream_);
    if (esc_stream_ != nullptr) (void)hipStreamDestroy(esc_stream_);
  }
}

// Set ctl.abort behind the kernel's back through the escape stream, so a
// scan loop that is still running stops at its next poll.
void ScanService::escalate_abort() {
  static const u32 one = 1;
  (void)hipMemcpyAsync(&d_svc_->ctl.abort, &one, sizeof(u32),
                       hipMemcpyHostToDevice, esc_stream_);
}

// Ask the resident kernel to exit and wait for it, bounded. The primary
// channel is the pinned quit_req word (a plain host store — always lands):
// the leader workgroup polls it between requests and broadcasts QUIT to
// the other workgroups through device stores (which, being on-device,
// cannot be blocked by anything). The hipMemcpy escalation is best-effort
// only: small H2D copies may be executed as blit kernels, which cannot get
// CUs while the persistent grid holds them.
bool ScanService::quit_bounded() {
  __atomic_store_n(&mb_->quit_req, 1u, __ATOMIC_RELEASE);
  const auto t0 = std::chrono::steady_clock::now();
  bool escalated = false;
  for (;;) {
    hipError_t q = hipStreamQuery(stream_);
    if (q != hipErrorNotReady) {
      running_ = false;
      mb_->quit_req = 0;
      return true;
    }
    const auto dt = std::chrono::steady_clock::now() - t0;
    if (!escalated && dt > std::chrono::seconds(5)) {
      escalated = true;
      static const u64 big_seq = ~0ULL;
      escalate_abort();
      (void)hipMemcpyAsync(&d_svc_->dev_seq, &big_seq, sizeof(u64),
                           hipMemcpyHostToDevice, esc_stream_);
    }
    if (dt > std::chrono::seconds(10)) return false;
    std::this_thread::yield();
  }
}

std::shared_ptr<ScanService> ScanService::acquire(int device, std::string* err) {
  std::lock_guard<std::mutex> lk(g_svc_mu);
  auto& slot = g_svc_registry[device];
  auto p = slot.lock();
  if (p != nullptr) return p;
  try {
    p = std::shared_ptr<ScanService>(new ScanService(device));
  } catch (const std::exception& e) {
    if (err != nullptr) *err = e.what();
    return nullptr;
  }
  slot = p;
  return p;
}

// answered: the sequence number of the last request that needs no serving
// any more; the kernel serves what the mailbox holds beyond it.
void ScanService::ensure_running_locked(u64 answered) {
  if (running_) {
    if (__atomic_load_n(&mb_->svc_state, __ATOMIC_ACQUIRE) == SVC_RUNNING) {
      return;
    }
    // The kernel retired itself; reap it.
    SBG_HIP_CHECK(hipStreamSynchronize(stream_));
    running_ = false;
  }
  SBG_HIP_CHECK(hipMemset(d_svc_, 0, SVC_DEV_CTL_BYTES));
  const u64 served0 = answered << 1;
  SBG_HIP_CHECK(hipMemcpy(&d_svc_->dev_seq, &served0, sizeof(u64),
                          hipMemcpyHostToDevice));
  mb_->quit_req = 0;
  mb_->alive = 0;
  __atomic_store_n(&mb_->svc_state, SVC_RUNNING, __ATOMIC_RELEASE);
  hipLaunchKernelGGL(k_scan4_service, dim3(grid_), dim3(SCAN_BLOCK), 0, stream_,
                     mb_, d_svc_, svc_idle_polls(), served0);
  SBG_HIP_CHECK(hipGetLastError());
  running_ = true;
  relaunches_ += 1;
  // Residency self-check: all workgroups must report in, otherwise the
  // completion protocol would deadlock. (Occupancy-API sizing should make
  // this impossible; a failure means something else holds CUs.)
  const auto t0 = std::chrono::steady_clock::now();
  while (__atomic_load_n(&mb_->alive, __ATOMIC_ACQUIRE) <
         static_cast<u32>(grid_)) {
    if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(2)) {
      const u32 alive = __atomic_load_n(&mb_->alive, __ATOMIC_ACQUIRE);
      if (svc_debug()) {
        std::fprintf(stderr, "[svc] residency failure: %u of %d alive\n", alive,
                     grid_);
      }
      quit_locked();
      throw std::runtime_error("scan service grid failed to become resident");
    }
    std::this_thread::yield();
  }
  if (svc_debug()) {
    std::fprintf(stderr, "[svc] launch #%llu: %d workgroups resident in %.1f us\n",
                 static_cast<unsigned long long>(relaunches_), grid_,
                 std::chrono::duration<double, std::micro>(
                     std::chrono::steady_clock::now() - t0)
                     .count());
  }
}

void ScanService::quit_locked() {
  if (!running_) return;
  if (!quit_bounded()) {
    throw std::runtime_error("scan service kernel refused to exit");
  }
}

void ScanService::park() {
  std::lock_guard<std::mutex> lk(mu_);
  if (!running_) return;
  (void)hipSetDevice(device_);
  if (__atomic_load_n(&mb_->svc_state, __ATOMIC_ACQUIRE) == SVC_RETIRED) {
    SBG_HIP_CHECK(hipStreamSynchronize(stream_));
    running_ = false;
    return;
  }
  quit_locked();
}

ScanResult ScanService::request(int op, const ScanRequest& rq, i64 begin,
                                i64 end) {
  std::lock_guard<std::mutex> lk(mu_);
  SBG_HIP_CHECK(hipSetDevice(device_));

  if (op == 2) {
    check_pair2_request(rq);
    fill_pair2_stage(&mb_->pair2_staging, rq);
  } else if (std::memcmp(&mb_->matcher_staging, rq.matcher,
                         sizeof(Avail3Matcher)) != 0) {
    // Matcher delta (content compare: pointers can be reused across engine
    // lifetimes, so identity alone is not a safe key).
    std::memcpy(&mb_->matcher_staging, rq.matcher, sizeof(Avail3Matcher));
    matcher_epoch_ += 1;
  }

  // Pool delta against the pinned shadow copy.
  int keep = 0;
  {
    const u64* a = reinterpret_cast<const u64*>(mb_->pool_staging);
    const u64* b = reinterpret_cast<const u64*>(rq.tables);
    const int limit = std::min(shadow_n_, rq.n) * 4;
    int i = 0;
    while (i < limit && a[i] == b[i]) i++;
    keep = i / 4;
    if (keep < rq.n) {
      std::memcpy(mb_->pool_staging + keep, rq.tables + keep,
                  sizeof(ttable) * static_cast<size_t>(rq.n - keep));
    }
    shadow_n_ = rq.n;
  }

  // Publish the request.
  const ttable T1 = rq.target & rq.mask;
  const ttable T0 = ~rq.target & rq.mask;
  mb_->hdr[HDR_N_KEEP] = static_cast<u64>(static_cast<u32>(rq.n)) |
                         (static_cast<u64>(static_cast<u32>(keep)) << 32);
  mb_->hdr[HDR_EPOCH_CALL] =
      static_cast<u64>(matcher_epoch_) |
      (static_cast<u64>(rq.count_all ? 1u : 0u) << 32);
  mb_->hdr[HDR_BEGIN] = static_cast<u64>(begin);
  mb_->hdr[HDR_END] = static_cast<u64>(end);
  mb_->hdr[HDR_OP] = static_cast<u64>(op);
  mb_->hdr[HDR_ORDERED] = op == 4 && rq.ordered && !rq.count_all ? 1 : 0;
  for (int w = 0; w < 4; w++) {
    mb_->hdr[HDR_T1 + w] = T1.w[w];
    mb_->hdr[HDR_T0 + w] = T0.w[w];
  }
  ensure_running_locked(seq_);
  const u64 s = ++seq_;
  __atomic_store_n(&mb_->req_seq, s, __ATOMIC_RELEASE);

  // Wait for the response. Every exit path is bounded: a retire race
  // relaunches, a stuck scan is aborted via the escape stream.
  const auto t0 = std::chrono::steady_clock::now();
  bool escalated = false;
  bool reported = false;
  int spins = 0;
  for (;;) {
    if (__atomic_load_n(&mb_->resp_seq, __ATOMIC_ACQUIRE) == s) break;
    if (__atomic_load_n(&mb_->svc_state, __ATOMIC_ACQUIRE) == SVC_RETIRED) {
      // The kernel retired just as we published: reap and relaunch; the
      // request is still in the mailbox and the fresh kernel serves it.
      SBG_HIP_CHECK(hipStreamSynchronize(stream_));
      running_ = false;
      ensure_running_locked(s - 1);
    }
    const auto dt = std::chrono::steady_clock::now() - t0;
    if (svc_debug() && !reported && dt > std::chrono::seconds(1)) {
      reported = true;
      std::fprintf(stderr,
                   "[svc] slow request: seq=%llu resp=%llu state=%u alive=%u "
                   "n=%d range=%lld\n",
                   static_cast<unsigned long long>(s),
                   static_cast<unsigned long long>(mb_->resp_seq),
                   mb_->svc_state, mb_->alive, rq.n,
                   static_cast<long long>(end - begin));
    }
    if (!escalated && dt > std::chrono::seconds(10)) {
      escalated = true;
      escalate_abort();
    }
    if (dt > std::chrono::seconds(20)) {
      quit_locked();
      throw std::runtime_error("scan service request timed out");
    }
    if (((spins++) & 0x3FF) == 0x3FF) std::this_thread::yield();
  }
  if (escalated) {
    quit_locked();
    throw std::runtime_error("scan service request needed an abort");
  }

  ScanResult out;
  out.evaluated = mb_->r_evaluated;
  if (out.evaluated > static_cast<u64>(end - begin)) {
    // A response that claims more work than the range is corruption;
    // treat it like a service failure (caller falls back to one-shot).
    quit_locked();
    throw std::runtime_error("scan service returned corrupt counts");
  }
  if (mb_->r_found != 0) {
    out.found = true;
    for (int i = 0; i < 10; i++) {
      out.res[i] = static_cast<u16>(mb_->r_res_w[i >> 2] >> ((i & 3) * 16));
    }
  }
  return out;
}

}  // namespace sbg
