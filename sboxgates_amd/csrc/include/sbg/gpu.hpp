// gpu.hpp — single-GPU scan engine: CDNA4 (gfx950) HIP kernels for the
// 3/5/7-LUT and shared-input two-LUT candidate scans and the gate-mode
// triple (k=4) and pair (k=2) scans. Implementation: csrc/hip/gpu_engine.hip
// (GpuEngine), csrc/hip/scan_launch.hpp (one-shot kernels) and
// csrc/hip/scan_service.hip (persistent k=4 / k=2 service).
//
// One GpuEngine owns one device (HIP_VISIBLE_DEVICES / torchrun LOCAL_RANK
// selects which): multi-GPU runs use one process per GPU with RCCL-backed
// coordination at the Engine/DistCtx layer, never inside this class.
#pragma once

#include <memory>
#include <string>

#include "sbg/scan.hpp"

namespace sbg {

// 5-LUT scan: a batch of triples whose longest row (the gates behind the
// triple's last one, m = n - 1 - c) exceeds this takes the wide walk, which
// screens the e's of a row one 32-gate word of the gate-transposed pool at a
// time; shorter rows keep the 4-pair row segments. Pools of at most
// SCAN5_WIDE_MIN_ROW + 3 gates therefore never reach the wide walk.
constexpr int SCAN5_WIDE_MIN_ROW = 40;
// 5-LUT scan: pools of at least this many gates run the wide kernel's
// wave-owned variant (k_scan5_wave), which walks every triple on the
// transposed pool and has no block barrier in its walk. Measured, full-range
// scans: 3 % less time than the batch kernel at 150 gates, 43 % at 180, 52 %
// at 220; more time below (11 % at 120 gates, 27 % at 90), where most
// triples have one or two steps and the chunk set-up is most of the work.
constexpr int SCAN5_WAVE_MIN_POOL = 150;
// 32-gate words of the transposed pool per wide task (1 or 2).
constexpr int SCAN5_WIDE_WORDS = 2;

class GpuEngine {
 public:
  // Returns nullptr when no HIP device is visible (err describes why).
  static std::unique_ptr<GpuEngine> create(int device, std::string* err);
  ~GpuEngine();

  // Scans combinations [begin, end) of C(rq.n, k), k in {2,3,4,5,7} (k=4
  // ranks triples), or of C(rq.n, 4) for k = SCAN_SHARED (one-shot kernel
  // k_scan4s, never the scan service). Blocking; early-exits via an in-kernel abort flag
  // unless rq.count_all, and then reports whichever hit won the election.
  // With rq.ordered it reports the hit of the lowest rank instead: found and
  // res[10] are exactly those of the matching cpu_scanK on the same window
  // (evaluated is then only known to lie in [1, window size]); a candidate
  // that hits on the GPU and misses on the CPU throws. k=2 is the pair
  // scan: it needs rq.matcher2, always reports the hit of the lowest rank
  // (see cpu_scan2) and, like k=4, goes through the scan service when that
  // is active.
  ScanResult scan(int k, const ScanRequest& rq, i64 begin, i64 end);

  // True when k=4 scans go through the persistent scan-service kernel
  // (~5-8 us per call) instead of one-shot launches (~30 us API floor).
  // Lazily creates the per-device service on first query.
  bool scan4_service_active();

  int device() const;
  std::string device_name() const;

  struct Impl;

 private:
  explicit GpuEngine(Impl* impl) : impl_(impl) {}
  Impl* impl_;
};

// True if the process can see at least one HIP device.
bool gpu_available();
int gpu_count();

// The smallest pool that runs k_scan5_wave, SCAN5_WAVE_MIN_POOL unless set
// otherwise; process-wide. For measuring the crossover and for tests that
// run the wave-owned kernel on small pools.
int scan5_wave_min_pool();
void set_scan5_wave_min_pool(int n);

}  // namespace sbg
