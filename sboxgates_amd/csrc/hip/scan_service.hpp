// scan_service.hpp — host interface of the persistent k=4 / k=2 scan service
// (implementation and kernel: scan_service.hip). Private to csrc/hip.
#pragma once

#include <hip/hip_runtime.h>

#include <memory>
#include <mutex>
#include <string>

#include "sbg/scan.hpp"

namespace sbg {

struct SvcMailbox;
struct SvcDev;

// ---------------------------------------------------------------------------
// ScanService — host side of the persistent scan kernel (k=4 triple scans
// and k=2 pair scans). One instance
// per device per process (gate-mode engines and --jobs workers share it;
// requests serialize on a mutex, which is correct because every request is
// a whole-device scan anyway).
// ---------------------------------------------------------------------------
class ScanService {
 public:
  static std::shared_ptr<ScanService> acquire(int device, std::string* err);
  ~ScanService();

  // Blocking k=4 scan via the resident kernel. Thread-safe.
  ScanResult scan4(const ScanRequest& rq, i64 begin, i64 end) {
    return request(4, rq, begin, end);
  }
  // Blocking k=2 pair scan via the same kernel, pool shadow and delta sync;
  // rq.matcher2 and rq.order travel with every request. Thread-safe.
  ScanResult scan2(const ScanRequest& rq, i64 begin, i64 end) {
    return request(2, rq, begin, end);
  }

  // Retire the resident kernel if it is running (used before launching
  // other kernels so an idle service never delays them). Cheap when the
  // kernel already retired itself.
  void park();

 private:
  explicit ScanService(int device);
  ScanResult request(int op, const ScanRequest& rq, i64 begin, i64 end);
  void ensure_running_locked(u64 answered);
  void quit_locked();
  bool quit_bounded();
  void escalate_abort();

  std::mutex mu_;
  int device_;
  hipStream_t stream_ = nullptr;      // service kernel lives here
  hipStream_t esc_stream_ = nullptr;  // escape-hatch async writes
  SvcMailbox* mb_ = nullptr;          // pinned fine-grained
  SvcDev* d_svc_ = nullptr;
  u64 seq_ = 0;
  u64 relaunches_ = 0;
  int grid_ = 0;
  bool running_ = false;
  int shadow_n_ = 0;                  // valid prefix of mb_->pool_staging
  u32 matcher_epoch_ = 0;
};

}  // namespace sbg
