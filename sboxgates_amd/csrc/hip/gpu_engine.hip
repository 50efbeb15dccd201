// gpu_engine.hip — GpuEngine (sbg/gpu.hpp), the host wrapper of the GPU
// scans. Host code only: one-shot scans go through the typed launchers of
// scan_launch.hpp, small k=4 / k=2 scans through the persistent service
// (scan_service.hpp).

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>

#include "sbg/comb.hpp"
#include "sbg/gpu.hpp"
#include "sbg/lutcover.hpp"
#include "sbg/scan5_geom.hpp"
#include "scan_launch.hpp"
#include "scan_service.hpp"

namespace sbg {

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

// Grid of a kernel that walks `items` with a grid stride.
static int strided_grid(u64 items) {
  return static_cast<int>(
      std::min<u64>((items + SCAN_BLOCK - 1) / SCAN_BLOCK, 4096));
}

// Grid of a kernel whose workgroups take `batch` units at a time off a queue
// of `units`. Sized to the unit count: small scans (deep recursion) pay for
// pool staging per block, so an always-2048 grid costs ~10x the useful work
// there.
static int queue_grid(i64 units, int batch) {
  return static_cast<int>(std::min<i64>((units + batch - 1) / batch + 1, 2048));
}

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

  // Zero h_ctl. lowest: the scan reports its lowest hit through best.
  void reset_ctl(bool lowest) {
    std::memset(h_ctl, 0, sizeof(DevCtl));
    if (lowest) h_ctl->best = ~0ULL;
  }

  // One launch round trip: upload h_ctl, launch, download h_ctl, wait.
  template <class Launch>
  void round_trip(Launch launch) {
    SBG_HIP_CHECK(hipMemcpyAsync(d_ctl, h_ctl, sizeof(DevCtl),
                                 hipMemcpyHostToDevice, stream));
    launch();
    SBG_HIP_CHECK(hipGetLastError());
    SBG_HIP_CHECK(hipMemcpyAsync(h_ctl, d_ctl, sizeof(DevCtl),
                                 hipMemcpyDeviceToHost, stream));
    SBG_HIP_CHECK(hipStreamSynchronize(stream));
  }
  void run(ScanKernel which, bool ordered, int grid, const ScanArgs& args) {
    round_trip([&] { launch_scan(which, ordered, grid, stream, args); });
  }

  bool service_active() {
    if (svc != nullptr) return true;
    if (svc_broken || svc_tried) return false;
    svc_tried = true;
    const char* off = std::getenv("SBOXGATES_NO_SVC");
    if (off != nullptr && off[0] != '\0' && off[0] != '0') {
      svc_broken = true;
      return false;
    }
    std::string err;
    svc = ScanService::acquire(device, &err);
    if (svc == nullptr) {
      svc_broken = true;
      return false;
    }
    return true;
  }

  // Service routing. The service takes only small and medium k=4 / k=2
  // ranges: its 64-WG grid is sized for the request/response round trip, not
  // for multi-million-candidate scans — those go to the one-shot kernel with
  // a work-sized grid. True: the service answered, *out is the scan's result.
  bool try_service(int k, const ScanRequest& rq, i64 begin, i64 end,
                   ScanResult* out) {
    if (k != 4 && k != 2) {
      // Do not let an idle-resident service delay other kernels.
      if (svc != nullptr) svc->park();
      return false;
    }
    if (end - begin > (1 << 20) || !service_active()) return false;
    try {
      *out = k == 4 ? svc->scan4(rq, begin, end) : svc->scan2(rq, begin, end);
      return true;
    } catch (const std::exception& e) {
      // Service failure (residency/timeout): permanently fall back to the
      // one-shot launch path for this engine.
      std::fprintf(stderr, "sboxgates: scan service disabled: %s\n", e.what());
      svc.reset();
      svc_broken = true;
      return false;
    }
  }

  // Upload the pool (through pinned staging), reset the control block
  // (lowest: see reset_ctl) and fill the kernels' arguments.
  ScanArgs stage(const ScanRequest& rq, i64 begin, i64 end, bool lowest) {
    std::memcpy(h_pool, rq.tables, sizeof(ttable) * rq.n);
    SBG_HIP_CHECK(hipMemcpyAsync(d_pool, h_pool, sizeof(ttable) * rq.n,
                                 hipMemcpyHostToDevice, stream));
    reset_ctl(lowest);
    ScanArgs args;
    args.pool = d_pool;
    args.ctl = d_ctl;
    args.hits = d_hits;
    args.hit_cap = hit_cap;
    args.matcher = d_matcher;
    args.pair2 = d_pair2;
    args.T1 = rq.target & rq.mask;
    args.T0 = ~rq.target & rq.mask;
    args.n = rq.n;
    args.begin = begin;
    args.end = end;
    args.excl = rq.excl_low64;
    args.seed = rq.seed;
    args.count_all = rq.count_all ? 1 : 0;
    args.slices7 = 1;
    return args;
  }

  // The strided kinds, k = 2, 3 and 4: one thread per rank, grid-stride.
  void run_strided(int k, const ScanRequest& rq, bool ordered,
                   const ScanArgs& args) {
    if (k == 2) {
      fill_pair2_stage(h_pair2, rq);
      SBG_HIP_CHECK(hipMemcpyAsync(d_pair2, h_pair2, sizeof(Pair2Stage),
                                   hipMemcpyHostToDevice, stream));
    } else if (k == 4 && last_matcher != rq.matcher) {
      // The matcher is per-engine and immutable; upload once.
      SBG_HIP_CHECK(hipMemcpy(d_matcher, rq.matcher, sizeof(Avail3Matcher),
                              hipMemcpyHostToDevice));
      last_matcher = rq.matcher;
    }
    run(k == 2 ? KERNEL_SCAN2 : (k == 3 ? KERNEL_SCAN3 : KERNEL_SCAN4),
        ordered, strided_grid(static_cast<u64>(args.end - args.begin)), args);
  }

  // The prefix-queue kinds, k = 5 and the shared-input scan: the queue of
  // triple prefixes is seeded at the triple containing `begin`.
  void run_prefix_queue(int k, const ScanRequest& rq, bool ordered,
                        const ScanArgs& args) {
    const bool shared = k == SCAN_SHARED;
    i64 t_begin, t_last;
    prefix_rank_span(rq.n, shared ? 4 : 5, 3, args.begin, args.end, &t_begin,
                     &t_last);
    const i64 units = t_last - t_begin + 1;
    if (!shared && rq.n >= scan5_wave_min_pool()) {
      // Large pools: the wide kernel whose waves own their triples. They
      // take chunks of the triples [t_begin, t_begin + units), numbered from
      // 0, at least SCAN5_CHUNK_MIN triples a wave.
      h_ctl->queue = 0;
      const int grid = queue_grid(units, SCAN5_CHUNK_MIN * (SCAN_BLOCK / 64));
      round_trip([&] {
        launch_scan5_wave(ordered, grid, stream, args, t_begin, units);
      });
      return;
    }
    h_ctl->queue = static_cast<unsigned long long>(t_begin);
    const int grid = queue_grid(units, shared ? SB : TB);
    // k=5: pools without a row longer than the crossover never take the wide
    // walk: they get the variant that has no transposed pool to build.
    const ScanKernel which =
        shared ? KERNEL_SCAN4S
               : (rq.n - 3 > SCAN5_WIDE_MIN_ROW ? KERNEL_SCAN5_WIDE
                                                : KERNEL_SCAN5_ROWS);
    run(which, ordered, grid, args);
  }

  // 7-LUT filter over [lo, hi), with overflow-driven range splitting: returns
  // the end of the range that fitted the hit buffer; h_ctl holds that
  // attempt's final state.
  i64 filter7(const ScanRequest& rq, bool ordered, ScanArgs args, i64 lo,
              i64 hi) {
    for (;;) {
      reset_ctl(ordered);
      if (ordered) h_ctl->pool_n = static_cast<u32>(rq.n);
      i64 q_begin, q_last;
      prefix_rank_span(rq.n, 7, 4, lo, hi, &q_begin, &q_last);
      const i64 qcount = q_last - q_begin + 1;
      // Sub-quad slicing: a single quad prefix can hold C(n-4,3) triples
      // (tens of thousands); without slicing a small scan runs on a
      // handful of blocks and leaves the chip idle.
      const i64 want_units = (hi - lo + SLICE_UNIT - 1) / SLICE_UNIT;
      const int slices = static_cast<int>(
          std::clamp<i64>(want_units / std::max<i64>(qcount, 1), 1, 256));
      args.begin = lo;
      args.end = hi;
      args.slices7 = slices;
      h_ctl->queue = static_cast<unsigned long long>(q_begin * slices);
      run(KERNEL_SCAN7_FILTER, false, queue_grid(qcount * slices, QB), args);
      if (h_ctl->overflow == 0) return hi;
      // Too many feasible combinations for the buffer: halve the range.
      hi = lo + (hi - lo) / 2;
      if (hi <= lo + 1) {
        throw std::runtime_error("7-LUT hit buffer too small for one combo");
      }
    }
  }

  // 7-LUT scan: filter + assign, sub-range by sub-range.
  ScanResult scan7(const ScanRequest& rq, bool ordered, ScanArgs args) {
    if (d_hits == nullptr) {
      SBG_HIP_CHECK(hipMalloc(&d_hits, sizeof(Hit7) * hit_cap));
    }
    args.hits = d_hits;
    ScanResult out;
    for (i64 lo = args.begin; lo < args.end;) {
      const i64 hi = filter7(rq, ordered, args, lo, args.end);
      // Accounting invariant: h_ctl is zeroed at the top of every attempt,
      // so only the final (non-overflowed) attempt's counter lands here —
      // combinations re-scanned after an overflow are never double-counted.
      out.evaluated += h_ctl->evaluated;
      const unsigned long long nhits =
          std::min<unsigned long long>(h_ctl->hit_count, hit_cap);
      if (nhits > 0 && !rq.count_all) {
        const u64 items = nhits * LUT7_NUM_ORDERINGS * FM_SPLIT;
        // h_ctl still holds the filter's final state, which the upload
        // puts back unchanged.
        round_trip([&] {
          launch_assign7(ordered, strided_grid(items), stream, d_hits, nhits,
                         d_ctl, rq.seed);
        });
        // Ordered: the sub-ranges come in increasing order, so the first one
        // with a hit holds the scan's lowest.
        const ScanResult r = result(7, rq, ordered, lo, hi, out.evaluated);
        if (r.found) return r;
      }
      lo = hi;
    }
    return out;
  }

  // The scan's result from what the kernels left in h_ctl.
  ScanResult result(int k, const ScanRequest& rq, bool ordered, i64 begin,
                    i64 end, u64 evaluated) const {
    const u64 best = h_ctl->best;
    if (k == 2) return pair2_result(best, rq, begin, end);
    if (ordered && best != ~0ULL) {
      return ordered_result(k, rq, k <= 4 ? best >> BEST3_SHIFT : best,
                            evaluated);
    }
    ScanResult out;
    out.evaluated = evaluated;
    if (h_ctl->found != 0) {
      out.found = true;
      std::memcpy(out.res, h_ctl->res, sizeof(out.res));
    }
    return out;
  }
};

bool gpu_available() { return gpu_count() > 0; }

static int g_scan5_wave_min_pool = SCAN5_WAVE_MIN_POOL;
int scan5_wave_min_pool() { return g_scan5_wave_min_pool; }
void set_scan5_wave_min_pool(int n) { g_scan5_wave_min_pool = n; }

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

bool GpuEngine::scan4_service_active() { return impl_->service_active(); }

ScanResult GpuEngine::scan(int k, const ScanRequest& rq, i64 begin, i64 end) {
  ScanResult out;
  // As cpu_scan2 and cpu_scan4s do.
  if ((k == 2 || k == SCAN_SHARED) && begin < 0) begin = 0;
  end = std::min(end, scan_space(rq.n, k));
  if (begin >= end) return out;

  Impl* im = impl_;
  SBG_HIP_CHECK(hipSetDevice(im->device));
  if (k == 2) check_pair2_request(rq);
  if (k == 4 && rq.matcher == nullptr) {
    throw std::runtime_error("scan4 needs matcher");
  }
  if (im->try_service(k, rq, begin, end, &out)) return out;

  // count_all ignores the option; the pair scan is ordered as it is.
  const bool ordered = rq.ordered && !rq.count_all && k != 2;
  const ScanArgs args = im->stage(rq, begin, end, ordered || k == 2);
  switch (k) {
    case 2:
    case 3:
    case 4: im->run_strided(k, rq, ordered, args); break;
    case 5:
    case SCAN_SHARED: im->run_prefix_queue(k, rq, ordered, args); break;
    case 7: return im->scan7(rq, ordered, args);
    default: throw std::runtime_error("GpuEngine::scan: bad k");
  }
  return im->result(k, rq, ordered, begin, end, im->h_ctl->evaluated);
}

}  // namespace sbg
