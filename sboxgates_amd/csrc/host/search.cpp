// search.cpp — Kwan's iterative gate-addition search, the LUT search and
// the multi-output beam driver. See search.hpp for parity notes.

#include "sbg/search.hpp"

#include <algorithm>
#include <cassert>
#include <thread>
#include <vector>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "sbg/comb.hpp"
#include "sbg/gpu.hpp"
#include "sbg/lutcover.hpp"
#include "sbg/xmlio.hpp"

namespace sbg {

// ---------------------------------------------------------------------------
// Gate-append primitives (parity: sboxgates.c:95-229).
// ---------------------------------------------------------------------------

gatenum add_gate(state* st, int type, gatenum gid1, gatenum gid2, metric_t metric) {
  assert(!(type == NOT && gid2 != NO_GATE));
  assert(type != IN && type != LUT);
  if (gid1 == NO_GATE || (gid2 == NO_GATE && type != NOT)) return NO_GATE;
  // Hard capacity check first: the reference's `num_gates > max_gates` test
  // alone writes one past gates[MAX_GATES-1] when max_gates == MAX_GATES
  // (the init_state default) and a mux chain reaches exactly MAX_GATES
  // gates — an out-of-bounds write in the reference; rejected here.
  if (st->num_gates >= MAX_GATES) return NO_GATE;
  if (st->num_gates > st->max_gates) return NO_GATE;
  if (metric == METRIC_SAT && st->sat_metric > st->max_sat_metric) return NO_GATE;
  assert(gid1 < st->num_gates);
  assert(gid2 < st->num_gates || type == NOT);
  assert(gid1 != gid2);

  st->sat_metric += sat_metric_of(type);
  gate& g = st->gates[st->num_gates];
  if (type == NOT) {
    g.table = ~st->gates[gid1].table;
  } else {
    g.table = gen_ttable_2(type, st->gates[gid1].table, st->gates[gid2].table);
  }
  g.type = type;
  g.in1 = gid1;
  g.in2 = gid2;
  g.in3 = NO_GATE;
  g.function = 0;
  st->num_gates += 1;
  return static_cast<gatenum>(st->num_gates - 1);
}

gatenum add_not_gate(state* st, gatenum gid, metric_t metric) {
  if (gid == NO_GATE) return NO_GATE;
  return add_gate(st, NOT, gid, NO_GATE, metric);
}

gatenum add_lut(state* st, u8 func, const ttable& table, gatenum g1, gatenum g2,
                gatenum g3) {
  if (g1 == NO_GATE || g2 == NO_GATE || g3 == NO_GATE ||
      st->num_gates >= MAX_GATES || st->num_gates > st->max_gates) {
    return NO_GATE;
  }
  assert(g1 < st->num_gates && g2 < st->num_gates && g3 < st->num_gates);
  assert(g1 != g2 && g2 != g3 && g3 != g1);
  gate& g = st->gates[st->num_gates];
  g.table = table;
  g.type = LUT;
  g.in1 = g1;
  g.in2 = g2;
  g.in3 = g3;
  g.function = func;
  st->num_gates += 1;
  return static_cast<gatenum>(st->num_gates - 1);
}

static gatenum add_and_gate(state* st, gatenum g1, gatenum g2, metric_t metric) {
  if (g1 == NO_GATE || g2 == NO_GATE) return NO_GATE;
  if (g1 == g2) return g1;
  return add_gate(st, AND, g1, g2, metric);
}

static gatenum add_or_gate(state* st, gatenum g1, gatenum g2, metric_t metric) {
  if (g1 == NO_GATE || g2 == NO_GATE) return NO_GATE;
  if (g1 == g2) return g1;
  return add_gate(st, OR, g1, g2, metric);
}

static gatenum add_xor_gate(state* st, gatenum g1, gatenum g2, metric_t metric) {
  if (g1 == NO_GATE || g2 == NO_GATE) return NO_GATE;
  // XOR(x, x) is constant FALSE — a degenerate multiplexer (both
  // half-space solutions equal the selector bit). The reference ABORTS
  // here (add_gate's gid1 != gid2 assert, sboxgates.c:103, reachable for
  // degenerate targets); skipping the variant lets the search continue.
  if (g1 == g2) return NO_GATE;
  return add_gate(st, XOR, g1, g2, metric);
}

gatenum add_boolfunc_2(state* st, const boolfunc& fun, gatenum g1, gatenum g2,
                       metric_t metric) {
  assert(fun.num_inputs == 2);
  if (g1 == NO_GATE || g2 == NO_GATE || st->num_gates > st->max_gates) return NO_GATE;
  if (metric == METRIC_SAT && st->sat_metric > st->max_sat_metric) return NO_GATE;
  if (fun.not_a) g1 = add_not_gate(st, g1, metric);
  if (fun.not_b) g2 = add_not_gate(st, g2, metric);
  gatenum gid = add_gate(st, fun.fun1, g1, g2, metric);
  if (fun.not_out) gid = add_not_gate(st, gid, metric);
  return gid;
}

gatenum add_boolfunc_3(state* st, const boolfunc& fun, gatenum g1, gatenum g2,
                       gatenum g3, metric_t metric) {
  if (g1 == NO_GATE || g2 == NO_GATE || (g3 == NO_GATE && fun.num_inputs == 3) ||
      st->num_gates > st->max_gates) {
    return NO_GATE;
  }
  if (metric == METRIC_SAT && st->sat_metric > st->max_sat_metric) return NO_GATE;
  if (fun.not_a) g1 = add_not_gate(st, g1, metric);
  if (fun.not_b) g2 = add_not_gate(st, g2, metric);
  if (fun.not_c) g3 = add_not_gate(st, g3, metric);
  gatenum out1 = add_gate(st, fun.fun1, g1, g2, metric);
  if (fun.not_out) {
    return add_not_gate(st, add_gate(st, fun.fun2, out1, g3, metric), metric);
  }
  return add_gate(st, fun.fun2, out1, g3, metric);
}

u8 eval_circuit(const state& st, u8 input) {
  // Straight DAG evaluation on a single input pattern — the ground-truth
  // oracle for tests (independent of cached truth tables).
  bool val[MAX_GATES];
  int ninputs = get_num_inputs(&st);
  for (int i = 0; i < st.num_gates; i++) {
    const gate& g = st.gates[i];
    switch (g.type) {
      case IN:
        val[i] = ((input >> i) & 1) != 0;
        break;
      case NOT:
        val[i] = !val[g.in1];
        break;
      case LUT: {
        int p = (val[g.in1] << 2) | (val[g.in2] << 1) | (val[g.in3] ? 1 : 0);
        val[i] = ((g.function >> p) & 1) != 0;
        break;
      }
      default: {
        int pat = ((val[g.in1] ? 1 : 0) << 1) | (val[g.in2] ? 1 : 0);
        val[i] = fun2_val(static_cast<u8>(g.type), static_cast<u8>(pat)) != 0;
        break;
      }
    }
  }
  (void)ninputs;
  u8 out = 0;
  for (int b = 0; b < 8; b++) {
    if (st.outputs[b] != NO_GATE && val[st.outputs[b]]) out |= 1u << b;
  }
  return out;
}

// ---------------------------------------------------------------------------
// Return-assertion (parity: ASSERT_AND_RETURN, sboxgates.h:31-44). A failed
// assertion indicates an engine/kernel bug; throw instead of abort so the
// Python bindings surface it loudly.
// ---------------------------------------------------------------------------
static gatenum assert_ret(gatenum ret, const ttable& target, const state* st,
                          const ttable& mask, const char* where) {
  if (ret == NO_GATE || tt_eq_mask(target, st->gates[ret].table, mask)) return ret;
  throw std::runtime_error(std::string("sboxgates: return assertion failed in ") +
                           where);
}

// ---------------------------------------------------------------------------
// Cell-requirement helpers for the step-3/4 scans: the forced function bits
// a candidate pair/triple imposes, and permutations thereof.
// ---------------------------------------------------------------------------

// Per-gate masked halves, precomputed once per node for the step-3/4a
// pair loops: p = t&T1, q = ~t&T1, r = t&T0, s = ~t&T0. A pair cell's
// masked content is then one AND of two halves ((±tx)&(±ty)&T1 =
// (±tx&T1)&(±ty&T1)), which removes the per-pair cell construction and
// the ~t materializations — the pair loops are ~60% of gate-mode host
// time (profiles/gate_mode_service.md).
struct GateHalves {
  ttable p, q, r, s;
};

static void fill_halves(GateHalves* out, const state* st, int n, const ttable& T1,
                        const ttable& T0) {
  for (int i = 0; i < n; i++) {
    const ttable& t = st->gates[i].table;
    out[i].p = t & T1;
    out[i].q = ~t & T1;
    out[i].r = t & T0;
    out[i].s = ~t & T0;
  }
}

// 4-cell requirements for a pair (x, y): bit p of req*/care is pattern
// p = vx<<1 | vy. Returns false if some cell is contradictory (no 2-input
// function can match). Kept out of line: on its own the compiler vectorizes
// the cells; inlined into the pair sweep it emits scalar code with spills
// and step 3 measured 6 % slower.
[[gnu::noinline]] static bool pair_requirements(const GateHalves& x,
                                                const GateHalves& y, u8* req1,
                                                u8* care) {
  u8 r1 = 0, r0 = 0;
  for (int p = 0; p < 4; p++) {
    bool has1 = tt_any((p & 2 ? x.p : x.q) & (p & 1 ? y.p : y.q));
    bool has0 = tt_any((p & 2 ? x.r : x.s) & (p & 1 ? y.r : y.s));
    if (has1 && has0) return false;
    if (has1) r1 |= 1u << p;
    if (has0) r0 |= 1u << p;
  }
  *req1 = r1;
  *care = static_cast<u8>(r1 | r0);
  return true;
}

// The calling thread's halves buffer. Step 3 fills it and step 4a of the same
// node reads it, both before step 5 recurses, so one per thread is enough.
static std::vector<GateHalves>& halves_scratch() {
  static thread_local std::vector<GateHalves> halves;
  return halves;
}

// The pair sweep of steps 3 and 4a: the first pair of gates, in visit order,
// that a function of `funs` (ended by num_inputs == 0) combines into the
// target, in either argument order. A match ends the sweep with what
// appending the function returned, which is NO_GATE when the bounds forbid
// the append; no match is an empty optional. Via 4-cell forced-bit
// requirements instead of per-function truth-table evaluation; masked
// equality (see header note).
static inline std::optional<gatenum> pair_sweep(
    state* st, const ttable& target, const ttable& mask, const GateHalves* halves,
    const gatenum* order, const boolfunc* funs, metric_t metric, const char* where) {
  for (int i = 0; i < st->num_gates; i++) {
    const gatenum gi = order[i];
    for (int k = i + 1; k < st->num_gates; k++) {
      const gatenum gk = order[k];
      u8 req1, care;
      if (!pair_requirements(halves[gi], halves[gk], &req1, &care)) continue;
      const u8 req1s = swap_pair_patterns(req1);
      const u8 cares = swap_pair_patterns(care);
      for (int m = 0; funs[m].num_inputs != 0; m++) {
        const u8 fpat = fun2_pattern_table(funs[m].fun);
        if ((fpat & care) == req1) {
          return assert_ret(add_boolfunc_2(st, funs[m], gi, gk, metric), target, st,
                            mask, where);
        }
        if (!funs[m].ab_commutative && (fpat & cares) == req1s) {
          return assert_ret(add_boolfunc_2(st, funs[m], gk, gi, metric), target, st,
                            mask, where);
        }
      }
    }
  }
  return std::nullopt;
}

// Adds its lifetime to a phase counter of SearchStats.
struct PhaseTimer {
  using clock = std::chrono::steady_clock;
  double* acc;
  clock::time_point t0 = clock::now();
  ~PhaseTimer() { *acc += std::chrono::duration<double>(clock::now() - t0).count(); }
};

// ---------------------------------------------------------------------------
// Engine
// ---------------------------------------------------------------------------

Engine::Engine(const options& opt, DistCtx* ctx)
    : opt_(opt), ctx_(ctx != nullptr ? ctx : &local_) {
  if (opt_.seeded) {
    // Distinct per-rank streams from one seed.
    rng_.seed_splitmix(opt_.seed + 0x100000001ULL * static_cast<u64>(ctx_->rank()));
  }
  if (opt_.gpu != GPU_OFF) {
    std::string err;
    gpu_ = GpuEngine::create(opt_.gpu_device, &err);
    if (gpu_ == nullptr && opt_.gpu == GPU_FORCE) {
      throw std::runtime_error("sboxgates: GPU required but unavailable: " + err);
    }
  }
}

Engine::~Engine() = default;

const Avail3Matcher* Engine::matcher3() {
  if (matcher_ == nullptr) {
    matcher_ = std::make_unique<Avail3Matcher>();
    u8 funs[256], costs[256];
    for (int i = 0; i < opt_.num_avail_3; i++) {
      const boolfunc& f = opt_.avail_3[i];
      funs[i] = f.fun;
      costs[i] = static_cast<u8>(2 + (f.not_a ? 1 : 0) + (f.not_b ? 1 : 0) +
                                 (f.not_c ? 1 : 0) + (f.not_out ? 1 : 0));
    }
    build_avail3_matcher(funs, costs, opt_.num_avail_3, matcher_.get());
  }
  return matcher_.get();
}

const Pair2Matcher* Engine::matcher2(bool nots) {
  std::unique_ptr<Pair2Matcher>& m = matcher2_[nots ? 1 : 0];
  if (m == nullptr) {
    m = std::make_unique<Pair2Matcher>();
    build_pair2_matcher(nots ? opt_.avail_not : opt_.avail_gates, m.get());
  }
  return m.get();
}

bool Engine::gpu_active() const { return gpu_ != nullptr; }

void Engine::set_sbox(const u8 sbox[256], int num_inputs) {
  std::memcpy(sbox_, sbox, 256);
  num_inputs_ = num_inputs;
  for (u8 i = 0; i < 8; i++) g_target_[i] = generate_target(i, sbox_);
  num_outputs_ = 0;
  for (int i = 7; i >= 0; i--) {
    if (tt_any(g_target_[i])) {
      num_outputs_ = i + 1;
      break;
    }
  }
}

// Pair scan dispatch: on the GPU when it is forced (by gpu or by
// gpu_pairs) or the window reaches the measured cutover. Its counters are
// its own: the k=3/4 totals feed the adaptive k=4 cutover.
ScanResult Engine::scan_pairs(const ScanRequest& rq, i64 begin, i64 end) {
  if (rq.matcher2 == nullptr) throw std::runtime_error("scan2 needs matcher2");
  const bool use_gpu =
      gpu_ != nullptr && (opt_.gpu == GPU_FORCE || opt_.gpu_pairs == PAIRS_FORCE ||
                          end - begin >= GPU_PAIRS_MIN);
  if (use_gpu) {
    stats_.pair_scans_gpu += 1;
    return gpu_->scan(2, rq, begin, end);
  }
  stats_.pair_scans_cpu += 1;
  return cpu_scan2(rq, begin, end);
}

ScanResult Engine::scan(int k, const ScanRequest& rq_in, i64 begin, i64 end) {
  if (k == 2) return scan_pairs(rq_in, begin, end);
  // options::ordered: the GPU scan answers as the CPU scan would, so which
  // side runs a scan below changes the time it takes and nothing else.
  ScanRequest rq = rq_in;
  rq.ordered = rq.ordered || opt_.ordered;
  // Per-k GPU cutover: per-combination cost grows steeply with k (a 7-LUT
  // feasibility check walks 128 cells vs 32 for 5-LUT and 8 for 3-LUT), so
  // the range size where the GPU (incl. ~20-40us launch+upload overhead)
  // beats the CPU differs by ~100x across kinds. Measured on the AES bit-0
  // search: a size-only 2^16 threshold left 2.1e9 7-LUT combos on the CPU
  // and tripled the wall time. k=4 scans go through the persistent scan
  // service (~5-8 us/call vs the ~30 us one-shot floor), which moves the
  // cutover well down.
  // k=4 via the scan service: adaptive cutover. The service round trip is
  // roughly constant (~SVC_US), while the CPU path's per-candidate cost
  // varies ~10x with mask sparsity; route to the GPU when the estimated
  // CPU time for the range exceeds the round trip. SBOXGATES_GPU_MIN4
  // pins a fixed threshold instead.
  static const i64 min4_fixed = [] {
    const char* s = std::getenv("SBOXGATES_GPU_MIN4");
    return s != nullptr ? std::strtoll(s, nullptr, 10) : -1;
  }();
  i64 min4 = min4_fixed;
  if (min4 < 0) {
    constexpr double SVC_US = 12e-6;
    const double rate = stats_.scan_seconds3_cpu > 1e-4
                            ? stats_.candidates3_cpu / stats_.scan_seconds3_cpu
                            : 2e8;
    min4 = std::clamp<i64>(static_cast<i64>(rate * SVC_US), 1024, 1 << 16);
  }
  const i64 gpu_min =
      k == 7 ? 256
             : (k == 5 ? 4096
                       : (k == SCAN_SHARED
                              ? GPU_SHARED_MIN
                              : (k == 4 && gpu_ != nullptr &&
                                         gpu_->scan4_service_active()
                                     ? min4
                                     : 1 << 14)));
  bool use_gpu = gpu_ != nullptr && (opt_.gpu == GPU_FORCE || end - begin >= gpu_min);
  const auto t0 = std::chrono::steady_clock::now();
  ScanResult r;
  if (use_gpu) {
    stats_.gpu_scans += 1;
    r = gpu_->scan(k, rq, begin, end);
  } else {
    stats_.cpu_scans += 1;
    switch (k) {
      case 3: r = cpu_scan3(rq, begin, end); break;
      case 4: r = cpu_scan4(rq, begin, end); break;
      case 5: r = cpu_scan5(rq, begin, end); break;
      case 7: r = cpu_scan7(rq, begin, end); break;
      case SCAN_SHARED: r = cpu_scan4s(rq, begin, end); break;
      default: throw std::runtime_error("bad scan k");
    }
  }
  const double dt =
      std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (!use_gpu && k <= 4) {
    stats_.candidates3_cpu += r.evaluated;
    stats_.scan_seconds3_cpu += dt;
  }
  switch (k) {
    case 3:
    case 4:
      stats_.candidates3 += r.evaluated;
      stats_.scan_seconds3 += dt;
      break;
    case 5:
      stats_.candidates5 += r.evaluated;
      stats_.scan_seconds5 += dt;
      break;
    case SCAN_SHARED:
      stats_.candidates4s += r.evaluated;
      stats_.scan_seconds4s += dt;
      break;
    default:
      stats_.candidates7 += r.evaluated;
      stats_.scan_seconds7 += dt;
      break;
  }
  if (opt_.verbosity >= 3) {
    std::printf("[%4d] scan%s: %lld candidates in %.3fs (%.3g cand/s)%s\n",
                ctx_->rank(),
                k == SCAN_SHARED ? "4s" : std::to_string(k).c_str(),
                static_cast<long long>(r.evaluated), dt,
                dt > 0 ? r.evaluated / dt : 0.0, r.found ? " HIT" : "");
  }
  return r;
}

// Chunked symmetric scan with cross-rank agreement each chunk. Every rank
// executes the same number of allreduce rounds (computed from the global
// combination count), so the protocol cannot deadlock — the redesign of the
// reference's Isend/Irecv/cancel protocol (lut.c:665-740) for RCCL.
bool Engine::dist_scan_chunked(int k, const ScanRequest& rq, u64 chunk, u16 res[10]) {
  const i64 total = n_choose_k(rq.n, k);
  const int W = ctx_->world();
  const int r = ctx_->rank();
  const i64 start = total * r / W;
  const i64 stop = total * (r + 1) / W;
  const i64 maxlen = (total + W - 1) / W;
  const i64 nchunks = chunk == 0 ? 1 : (maxlen + static_cast<i64>(chunk) - 1) /
                                           static_cast<i64>(chunk);

  bool found_local = false;
  i64 pos = start;
  for (i64 c = 0; c < nchunks; c++) {
    if (!found_local && pos < stop) {
      i64 e = chunk == 0 ? stop : std::min(stop, pos + static_cast<i64>(chunk));
      ScanResult rr = scan(k, rq, pos, e);
      pos = e;
      if (rr.found) {
        found_local = true;
        std::memcpy(res, rr.res, sizeof(u16) * 10);
      }
    }
    if (W > 1) {
      int winner = ctx_->allreduce_min(found_local ? r : INT_MAX);
      if (winner != INT_MAX) {
        ctx_->bcast(res, sizeof(u16) * 10, winner);
        return true;
      }
    } else if (found_local) {
      return true;
    }
  }
  return false;
}

bool Engine::distributed_lut_body(const WorkMsg& w, u16 res[10], bool* found5) {
  // Build the pool view. The tables live inside the (broadcast) state.
  static thread_local std::vector<ttable> pool;
  const ScanRequest rq = make_scan_request(pool, w.st, w.target, w.mask, w.seed,
                                           excl_from_inbits(w.inbits));

  *found5 = false;
  // 5/7-LUT chunk sizes: fixed constants (env-overridable for tests) so
  // every rank derives the same chunk count from the broadcast state.
  static const u64 CHUNK5 = [] {
    const char* s = std::getenv("SBOXGATES_CHUNK5");
    return s != nullptr ? std::strtoull(s, nullptr, 10) : (1ULL << 30);
  }();
  static const u64 CHUNK7 = [] {
    const char* s = std::getenv("SBOXGATES_CHUNK7");
    return s != nullptr ? std::strtoull(s, nullptr, 10) : (1ULL << 30);
  }();
  if (w.st.num_gates >= 5) {
    if (w.verbosity >= 2 && ctx_->rank() == 0) std::printf("[   0] Search 5.\n");
    if (dist_scan_chunked(5, rq, CHUNK5, res)) {
      *found5 = true;
      return true;
    }
  }
  // 7-LUT phase; the gate check is symmetric (same broadcast state).
  if (!check_num_gates_possible(&w.st, 3, 0, METRIC_GATES)) return false;
  if (w.st.num_gates >= 7) {
    if (w.verbosity >= 2 && ctx_->rank() == 0) std::printf("[   0] Search 7.\n");
    return dist_scan_chunked(7, rq, CHUNK7, res);
  }
  return false;
}

void Engine::worker_loop() {
  // Parity: sboxgates.c:618-642 — block on broadcast work until quit.
  for (;;) {
    WorkMsg w;
    ctx_->bcast(&w, sizeof(WorkMsg), 0);
    if (w.kind == WORK_QUIT) return;
    u16 res[10];
    bool found5;
    distributed_lut_body(w, res, &found5);
  }
}

void Engine::stop_workers() {
  if (ctx_->world() <= 1 || ctx_->rank() != 0) return;
  WorkMsg w;
  std::memset(&w, 0, sizeof(w));
  w.kind = WORK_QUIT;
  ctx_->bcast(&w, sizeof(WorkMsg), 0);
}

// Appends the two LUTs of a result in the 5-LUT layout (a 5-LUT hit or a
// shared-input hit): res[0]=fo over gates res[2..4], res[1]=fi over that
// LUT and gates res[5], res[6].
static gatenum add_lut_pair(state* st, const u16 res[10], const ttable& target,
                            const ttable& mask, const char* where) {
  const u8 fo = static_cast<u8>(res[0]);
  const u8 fi = static_cast<u8>(res[1]);
  const ttable ta = st->gates[res[2]].table;
  const ttable tb = st->gates[res[3]].table;
  const ttable tc = st->gates[res[4]].table;
  const ttable td = st->gates[res[5]].table;
  const ttable te = st->gates[res[6]].table;
  ttable t_outer = gen_lut_ttable(fo, ta, tb, tc);
  ttable t_inner = gen_lut_ttable(fi, t_outer, td, te);
  return assert_ret(
      add_lut(st, fi, t_inner, add_lut(st, fo, t_outer, res[2], res[3], res[4]),
              res[5], res[6]),
      target, st, mask, where);
}

gatenum Engine::lut_search(state* st, const ttable& target, const ttable& mask,
                           const i8* inbits) {
  // --- 3-LUT scan (local to rank 0; parity: lut.c:501-523). ---
  {
    static thread_local std::vector<ttable> pool;
    // No exclusions: reference parity, the 3-LUT scan ignores inbits.
    const ScanRequest rq = make_scan_request(pool, *st, target, mask, rng_.next());
    ScanResult r = scan(3, rq, 0, n_choose_k(rq.n, 3));
    if (r.found) {
      const ttable& ta = st->gates[r.res[1]].table;
      const ttable& tb = st->gates[r.res[2]].table;
      const ttable& tc = st->gates[r.res[3]].table;
      ttable nt = gen_lut_ttable(static_cast<u8>(r.res[0]), ta, tb, tc);
      return assert_ret(
          add_lut(st, static_cast<u8>(r.res[0]), nt, r.res[1], r.res[2], r.res[3]),
          target, st, mask, "lut_search/3");
    }
  }

  if (!check_num_gates_possible(st, 2, 0, opt_.metric)) return NO_GATE;

  // --- Shared-input two-LUT scan (options::lut_shared; local to rank 0):
  // LUT(LUT(x,y,z), d, s) with s one of x, y, z, over all of C(n,4). Costs
  // the two LUTs of a 5-LUT hit and is assembled like one. ---
  if (opt_.lut_shared && st->num_gates >= 4) {
    static thread_local std::vector<ttable> pool;
    const ScanRequest rq = make_scan_request(pool, *st, target, mask, rng_.next(),
                                             excl_from_inbits(inbits));
    ScanResult r = scan(SCAN_SHARED, rq, 0, n_choose_k(rq.n, 4));
    if (r.found) {
      stats_.shared_hits += 1;
      if (opt_.verbosity >= 1) {
        std::printf("[%4d]   Selected 4LUT-shared: %02x %02x    %3d %3d %3d %3d %3d\n",
                    ctx_->rank(), r.res[0], r.res[1], r.res[2], r.res[3], r.res[4],
                    r.res[5], r.res[6]);
      }
      return add_lut_pair(st, r.res, target, mask, "lut_search/4s");
    }
  }

  // --- Distributed 5/7-LUT search (parity: lut.c:525-631). ---
  WorkMsg w;
  std::memset(&w, 0, sizeof(w));
  w.kind = WORK_LUT_SEARCH;
  w.verbosity = opt_.verbosity;
  w.seed = rng_.next();
  w.target = target;
  w.mask = mask;
  std::memcpy(w.inbits, inbits, 8);
  w.st = *st;
  if (ctx_->world() > 1) ctx_->bcast(&w, sizeof(WorkMsg), 0);

  u16 res[10];
  bool found5 = false;
  bool found = distributed_lut_body(w, res, &found5);
  if (found && found5) {
    if (opt_.verbosity >= 1) {
      std::printf("[%4d]   Selected 5LUT: %02x %02x    %3d %3d %3d %3d %3d\n",
                  ctx_->rank(), res[0], res[1], res[2], res[3], res[4], res[5],
                  res[6]);
    }
    return add_lut_pair(st, res, target, mask, "lut_search/5");
  }
  if (found) {
    u8 fo = static_cast<u8>(res[0]);
    u8 fm = static_cast<u8>(res[1]);
    u8 fi = static_cast<u8>(res[2]);
    if (opt_.verbosity >= 1) {
      std::printf("[%4d]   Selected 7LUT: %02x %02x %02x %3d %3d %3d %3d %3d %3d %3d\n",
                  ctx_->rank(), fo, fm, fi, res[3], res[4], res[5], res[6], res[7],
                  res[8], res[9]);
    }
    ttable t_outer = gen_lut_ttable(fo, st->gates[res[3]].table,
                                    st->gates[res[4]].table, st->gates[res[5]].table);
    ttable t_middle = gen_lut_ttable(fm, st->gates[res[6]].table,
                                     st->gates[res[7]].table, st->gates[res[8]].table);
    ttable t_inner = gen_lut_ttable(fi, t_outer, t_middle, st->gates[res[9]].table);
    return assert_ret(
        add_lut(st, fi, t_inner, add_lut(st, fo, t_outer, res[3], res[4], res[5]),
                add_lut(st, fm, t_middle, res[6], res[7], res[8]), res[9]),
        target, st, mask, "lut_search/7");
  }
  if (opt_.verbosity >= 2) {
    std::printf("[%4d] No LUTs found. Num gates: %d\n", ctx_->rank(),
                st->num_gates - get_num_inputs(st));
  }
  return NO_GATE;
}

// ---------------------------------------------------------------------------
// create_circuit: one recursion node of Kwan's algorithm.
// ---------------------------------------------------------------------------

// Step 1: an existing gate already realizes the map (sboxgates.c:301-308).
static std::optional<gatenum> step1_existing(state* st, const ttable& target,
                                             const ttable& mask,
                                             const gatenum* order) {
  for (int i = 0; i < st->num_gates; i++) {
    if (tt_eq_mask(target, st->gates[order[i]].table, mask)) {
      return assert_ret(order[i], target, st, mask, "step1");
    }
  }
  return std::nullopt;
}

// Step 2: an inverse realizes the map -> append NOT (sboxgates.c:310-321).
static std::optional<gatenum> step2_inverted(state* st, const ttable& target,
                                             const ttable& mask,
                                             const gatenum* order, metric_t metric) {
  if (!check_num_gates_possible(st, 1, sat_metric_of(NOT), metric)) return NO_GATE;
  for (int i = 0; i < st->num_gates; i++) {
    if (tt_eq_mask(target, ~st->gates[order[i]].table, mask)) {
      return assert_ret(add_not_gate(st, order[i], metric), target, st, mask, "step2");
    }
  }
  return std::nullopt;
}

gatenum Engine::create_circuit(state* st, const ttable& target, const ttable& mask,
                               const i8* inbits) {
  gatenum order[MAX_GATES];
  order_gates(*st, order);
  stats_.nodes += 1;

  std::optional<gatenum> done;
  {
    PhaseTimer timer{&stats_.step12_seconds};
    if ((done = step1_existing(st, target, mask, order))) return *done;
    if ((done = step2_inverted(st, target, mask, order, opt_.metric))) return *done;
  }
  if ((done = step3_pairs(st, target, mask, order))) return *done;
  if (opt_.lut_graph) {
    gatenum ret = lut_search(st, target, mask, inbits);
    if (ret != NO_GATE) return assert_ret(ret, target, st, mask, "lut_search");
  } else {
    if ((done = step4a_not_pairs(st, target, mask, order))) return *done;
    if ((done = step4b_triples(st, target, mask))) return *done;
  }
  return step5_multiplex(st, target, mask, inbits);
}

// Randomized gate visit order (parity: sboxgates.c:285-299).
void Engine::order_gates(const state& st, gatenum* order) {
  for (int i = 0; i < st.num_gates; i++) {
    order[i] = static_cast<gatenum>(st.num_gates - 1 - i);
  }
  if (opt_.randomize) {
    for (u32 i = st.num_gates - 1; i > 0; i--) {
      std::swap(order[i], order[rng_.below(i + 1)]);
    }
  }
}

// Step 3: a pair combined by one available gate (sboxgates.c:323-350).
std::optional<gatenum> Engine::step3_pairs(state* st, const ttable& target,
                                           const ttable& mask, const gatenum* order) {
  if (!check_num_gates_possible(st, 1, sat_metric_of(AND), opt_.metric)) {
    return NO_GATE;
  }
  if (pairs_on_gpu(st->num_gates)) {
    PhaseTimer timer{&stats_.step3_seconds};
    return pair_scan(st, target, mask, order, false, "step3");
  }
  std::vector<GateHalves>& halves = halves_scratch();
  halves.resize(st->num_gates);
  fill_halves(halves.data(), st, st->num_gates, target & mask, ~target & mask);
  PhaseTimer timer{&stats_.step3_seconds};
  return pair_sweep(st, target, mask, halves.data(), order, opt_.avail_gates,
                    opt_.metric, "step3");
}

// A function of n only, so steps 3 and 4a of a node decide alike: step 4a's
// host sweep needs the halves that step 3's host sweep left.
bool Engine::pairs_on_gpu(int n) const {
  if (gpu_ == nullptr || opt_.gpu_pairs == PAIRS_OFF) return false;
  return opt_.gpu_pairs == PAIRS_FORCE || n_choose_k(n, 2) >= GPU_PAIRS_MIN;
}

// The sweep as a k=2 scan in the node's visit order; the hit is the host
// sweep's first match and is appended the same way. Draws no random numbers.
std::optional<gatenum> Engine::pair_scan(state* st, const ttable& target,
                                         const ttable& mask, const gatenum* order,
                                         bool nots, const char* where) {
  static thread_local std::vector<ttable> pool;
  ScanRequest rq = make_scan_request(pool, *st, target, mask, 0);
  rq.matcher2 = matcher2(nots);
  rq.order = order;
  const ScanResult r = scan(2, rq, 0, n_choose_k(rq.n, 2));
  if (!r.found) return std::nullopt;
  const boolfunc* funs = nots ? opt_.avail_not : opt_.avail_gates;
  return assert_ret(
      add_boolfunc_2(st, funs[r.res[0]], r.res[2], r.res[3], opt_.metric), target,
      st, mask, where);
}

// Step 4a: pairs with NOT-augmented functions (sboxgates.c:358-386), over
// the halves that step 3 left.
std::optional<gatenum> Engine::step4a_not_pairs(state* st, const ttable& target,
                                                const ttable& mask,
                                                const gatenum* order) {
  if (!check_num_gates_possible(st, 2, sat_metric_of(AND) + sat_metric_of(NOT),
                                opt_.metric)) {
    return NO_GATE;
  }
  // Without -n the NOT-augmented function list is empty: the whole pair
  // sweep would compute requirements for zero candidate functions (the
  // reference pays this too, sboxgates.c:366-386 — measured at 22 s of
  // the AES bit-0 CPU run).
  if (opt_.avail_not[0].num_inputs == 0) return std::nullopt;
  PhaseTimer timer{&stats_.step4a_seconds};
  if (pairs_on_gpu(st->num_gates)) {
    return pair_scan(st, target, mask, order, true, "step4a");
  }
  return pair_sweep(st, target, mask, halves_scratch().data(), order,
                    opt_.avail_not, opt_.metric, "step4a");
}

// Step 4b: triples realized by an available composed 3-input function
// (sboxgates.c:388-435) — the gate-mode hot loop, run as a k=4 scan
// (GPU kernel k_scan4 on large pools): cell-requirement screen + one
// matcher-bitmap probe per argument order; all 6 orders (improvement
// over the reference's 4 orders with mis-indexed commutativity gates).
std::optional<gatenum> Engine::step4b_triples(state* st, const ttable& target,
                                              const ttable& mask) {
  if (!check_num_gates_possible(st, 3, 2 * sat_metric_of(AND) + sat_metric_of(NOT),
                                opt_.metric)) {
    return NO_GATE;
  }
  if (opt_.num_avail_3 <= 0 || st->num_gates < 3) return std::nullopt;
  static thread_local std::vector<ttable> pool;
  const ScanRequest rq =
      make_scan_request(pool, *st, target, mask, rng_.next(), 0, matcher3());
  ScanResult r = scan(4, rq, 0, n_choose_k(rq.n, 3));
  if (!r.found) return std::nullopt;
  const boolfunc& f = opt_.avail_3[r.res[0]];
  const int* sel = TRIPLE_PERMS6[r.res[1]];
  const gatenum ids[3] = {r.res[2], r.res[3], r.res[4]};
  return assert_ret(
      add_boolfunc_3(st, f, ids[sel[0]], ids[sel[1]], ids[sel[2]], opt_.metric),
      target, st, mask, "step4b");
}

// Cross-bit branch-and-bound of step 5 (gate mode): once an earlier bit
// produced `best`, later bits' candidates are only ever KEPT when strictly
// smaller (ties keep the first), so bound their sub-searches to strictly
// fewer gates. Measured: 3.4x fewer recursion nodes / 3.4x wall on AES
// bit 0 (186 s -> 55 s CPU-only), at a ~0.4-gate mean cost on single-shot
// runs (the tight bound reorders the greedy exploration) that -i 2 at the
// higher speed more than recovers. Not applied in LUT mode (its searches
// are scan-dominated; quality of the headline LUT artifacts stays
// byte-for-byte reproducible) nor under the SAT metric (its bound check is
// pre-append, so a tight bound would not be strict).
// SBOXGATES_NO_PRUNE=1 disables.
static gatenum cross_bit_bound(const options& opt, const state& best) {
  static const bool prune_off = [] {
    const char* e = std::getenv("SBOXGATES_NO_PRUNE");
    return e != nullptr && e[0] != '\0' && e[0] != '0';
  }();
  const bool prune = !prune_off && opt.metric == METRIC_GATES && !opt.lut_graph &&
                     best.num_gates >= 2;
  return prune ? static_cast<gatenum>(best.num_gates - 2) : MAX_GATES;
}

// Step 5: multiplex on an input bit and recurse on the half-spaces
// (sboxgates.c:438-607).
gatenum Engine::step5_multiplex(state* st, const ttable& target, const ttable& mask,
                                const i8* inbits) {
  i8 next_inbits[8];
  u8 bitp = 0;
  while (bitp < 6 && inbits[bitp] != -1) {
    next_inbits[bitp] = inbits[bitp];
    bitp += 1;
  }
  next_inbits[bitp] = -1;
  next_inbits[bitp + 1] = -1;

  // best.num_gates == 0 (gates metric) or best.sat_metric == 0 (SAT metric)
  // is "nothing kept yet".
  state best;
  gatenum best_out = NO_GATE;
  best.num_gates = 0;
  best.sat_metric = 0;

  for (int bit = 0; bit < get_num_inputs(st); bit++) {
    if (std::find(inbits, inbits + bitp, bit) != inbits + bitp) continue;
    next_inbits[bitp] = static_cast<i8>(bit);

    state nst;
    const gatenum bound = cross_bit_bound(opt_, best);
    const gatenum nst_out =
        opt_.lut_graph ? mux_lut(*st, target, mask, bit, bound, next_inbits, &nst)
                       : mux_and_or(*st, target, mask, bit, bound, next_inbits, &nst);
    if (nst_out == NO_GATE) continue;

    // Keep the best sub-state by the active metric (sboxgates.c:593-606).
    if (metric_value(best, opt_.metric) == 0 ||
        metric_value(nst, opt_.metric) < metric_value(best, opt_.metric)) {
      copy_state(best, nst);
      best_out = nst_out;
    }
  }

  if (best.num_gates == 0) return NO_GATE;
  copy_state(*st, best);
  return assert_ret(best_out, target, st, mask, "step5");
}

// LUT-based multiplexer: both halves built in one state, joined by a 0xac
// LUT unless a half is the selection bit itself.
gatenum Engine::mux_lut(const state& st, const ttable& target, const ttable& mask,
                        int bit, gatenum bound, const i8* next_inbits, state* nst) {
  const ttable fsel = st.gates[bit].table;  // selection bit
  copy_state(*nst, st);
  if (nst->max_gates > bound) nst->max_gates = bound;
  nst->max_gates -= 1;  // Room for the multiplexer.
  gatenum fb = create_circuit(nst, target, mask & ~fsel, next_inbits);
  if (fb == NO_GATE) return NO_GATE;
  gatenum fc = create_circuit(nst, target, mask & fsel, next_inbits);
  if (fc == NO_GATE) return NO_GATE;
  nst->max_gates = st.max_gates;  // restore the caller's bound exactly
                                  // (it was clamped by bound)

  gatenum out;
  if (fb == fc) {
    out = fb;
  } else if (fb == bit) {
    out = add_and_gate(nst, fb, fc, opt_.metric);
  } else if (fc == bit) {
    out = add_or_gate(nst, fb, fc, opt_.metric);
  } else {
    ttable mux_table = gen_lut_ttable(0xac, nst->gates[bit].table,
                                      nst->gates[fb].table, nst->gates[fc].table);
    out = add_lut(nst, 0xac, mux_table, static_cast<gatenum>(bit), fb, fc);
  }
  assert(out == NO_GATE || tt_eq_mask(target, nst->gates[out].table, mask));
  return out;
}

// Tries both the AND- and the OR-based multiplexer and keeps the smaller.
// The two do not treat their bounds alike, and searches depend on it.
gatenum Engine::mux_and_or(const state& st, const ttable& target, const ttable& mask,
                           int bit, gatenum bound, const i8* next_inbits,
                           state* nst) {
  const ttable fsel = st.gates[bit].table;  // selection bit
  state nst_and;
  copy_state(nst_and, st);
  if (nst_and.max_gates > bound) nst_and.max_gates = bound;
  nst_and.max_gates -= 2;
  nst_and.max_sat_metric -= sat_metric_of(AND) + sat_metric_of(XOR);

  gatenum mux_out_and = NO_GATE;
  gatenum fb = create_circuit(&nst_and, target & ~fsel, mask & ~fsel, next_inbits);
  if (fb != NO_GATE) {
    gatenum fc = create_circuit(&nst_and, nst_and.gates[fb].table ^ target,
                                mask & fsel, next_inbits);
    // The AND side goes back to the caller's gate bound outright (it was
    // clamped by bound) before its two appends; its SAT bound by addition.
    nst_and.max_gates = st.max_gates;
    nst_and.max_sat_metric += sat_metric_of(AND) + sat_metric_of(XOR);
    gatenum andg = add_and_gate(&nst_and, fc, static_cast<gatenum>(bit), opt_.metric);
    mux_out_and = add_xor_gate(&nst_and, fb, andg, opt_.metric);
  }

  state nst_or;
  copy_state(nst_or, st);
  if (nst_or.max_gates > bound) nst_or.max_gates = bound;
  // The OR side only has to beat the AND side, when that gave a result:
  // both of its bounds then come from nst_and, not from the caller.
  if (mux_out_and != NO_GATE) {
    nst_or.max_gates = nst_and.num_gates;
    nst_or.max_sat_metric = nst_and.sat_metric;
  }
  nst_or.max_gates -= 2;
  nst_or.max_sat_metric -= sat_metric_of(OR) + sat_metric_of(XOR);

  gatenum mux_out_or = NO_GATE;
  gatenum fd = create_circuit(&nst_or, ~target & fsel, mask & fsel, next_inbits);
  if (fd != NO_GATE) {
    gatenum fe = create_circuit(&nst_or, nst_or.gates[fd].table ^ target,
                                mask & ~fsel, next_inbits);
    // Unlike the AND side, the OR side appends under its own bounds,
    // restored by += 2, and takes the caller's only after the appends.
    nst_or.max_gates += 2;
    nst_or.max_sat_metric += sat_metric_of(OR) + sat_metric_of(XOR);
    gatenum org = add_or_gate(&nst_or, fe, static_cast<gatenum>(bit), opt_.metric);
    mux_out_or = add_xor_gate(&nst_or, fd, org, opt_.metric);
    nst_or.max_gates = st.max_gates;
    nst_or.max_sat_metric = st.max_sat_metric;
  }
  if (mux_out_and == NO_GATE && mux_out_or == NO_GATE) return NO_GATE;

  const bool pick_and =
      mux_out_or == NO_GATE ||
      (mux_out_and != NO_GATE &&
       metric_value(nst_and, opt_.metric) < metric_value(nst_or, opt_.metric));
  copy_state(*nst, pick_and ? nst_and : nst_or);
  return pick_and ? mux_out_and : mux_out_or;
}

// ---------------------------------------------------------------------------
// Drivers
// ---------------------------------------------------------------------------

void Engine::save_checkpoint(const state& st) {
  if (!opt_.save_states) return;
  std::string path = save_state(st, opt_.output_dir);
  if (!path.empty()) saved_files_.push_back(path);
}

std::optional<state> Engine::search_output(const state& start, int output) {
  std::optional<state> st(start);
  i8 bits[8] = {-1, -1, -1, -1, -1, -1, -1, -1};
  const ttable mask = tt_mask_for_inputs(get_num_inputs(&start));
  const gatenum out = create_circuit(&*st, g_target_[output], mask, bits);
  if (out == NO_GATE) return std::nullopt;
  assert(tt_eq_mask(g_target_[output], st->gates[out].table, mask));
  st->outputs[output] = out;
  return st;
}

// A worker engine has this engine's options with jobs = 1, no output, the
// job's seed, and the GPU at the job's place in its batch modulo the devices.
void Engine::run_jobs(const std::vector<Job>& jobs,
                      const std::function<void(Engine&, int)>& job,
                      const std::function<void(int, int)>& after_batch) {
  const int n = static_cast<int>(jobs.size());
  const int devices = gpu_ != nullptr ? std::max(1, gpu_count()) : 0;
  for (int first = 0; first < n; first += opt_.jobs) {
    const int count = std::min(opt_.jobs, n - first);
    std::vector<std::thread> threads;
    for (int j = 0; j < count; j++) {
      threads.emplace_back([&, first, j] {
        const int t = first + j;
        options wopt = opt_;
        wopt.jobs = 1;
        wopt.verbosity = -1;
        if (wopt.seeded) wopt.seed = jobs[t].seed;
        if (devices > 0) wopt.gpu_device = j % devices;
        try {
          Engine we(wopt);
          we.set_sbox(sbox_, num_inputs_);
          job(we, t);
        } catch (const std::exception& e) {
          std::fprintf(stderr, "%s failed: %s\n", jobs[t].name.c_str(), e.what());
        }
      });
    }
    for (auto& t : threads) t.join();
    if (after_batch) after_batch(first, count);
  }
}

// The end of iteration `index` (from 1) of a single-output search: report
// it, checkpoint what it found and tighten st's bound from that.
void Engine::finish_iteration(int index, const std::optional<state>& found,
                              state* st) {
  if (!found) {
    if (opt_.verbosity >= 0) {
      std::printf("(%d/%d): Not found.\n", index, opt_.iterations);
    }
    return;
  }
  if (opt_.verbosity >= 0) {
    std::printf("(%d/%d): %d gates. SAT metric: %d\n", index, opt_.iterations,
                found->num_gates - get_num_inputs(&*found), found->sat_metric);
  }
  save_checkpoint(*found);
  tighten_bound(*st, *found, opt_.metric);
}

void Engine::generate_graph_one_output(const state& st_in) {
  assert(opt_.iterations > 0);
  state st = st_in;
  if (opt_.jobs <= 1 || ctx_->world() != 1) {
    // Parity: sboxgates.c:661-688.
    if (opt_.verbosity >= 0) {
      std::printf("Generating graphs for output %d...\n", opt_.oneoutput);
    }
    for (int iter = 0; iter < opt_.iterations; iter++) {
      finish_iteration(iter + 1, search_output(st, opt_.oneoutput), &st);
    }
    return;
  }
  // Parallel independent iterations: batches of `jobs` threads, each with
  // its own engine (rotating over visible GPUs when present); search bounds
  // tighten between batches. Semantics: the same iteration count as the
  // serial driver, with bound tightening at batch granularity instead of
  // per-iteration — every produced circuit is identical in kind and
  // checkpointed the same way.
  if (opt_.verbosity >= 0) {
    std::printf("Generating graphs for output %d (%d parallel jobs)...\n",
                opt_.oneoutput, opt_.jobs);
  }
  std::vector<Job> jobs;
  for (int t = 0; t < opt_.iterations; t++) {
    jobs.push_back({opt_.seed + 0x9E37 * (t + 1), "search job " + std::to_string(t)});
  }
  // One slot per thread of a batch: iteration t uses slot t % opt_.jobs.
  std::vector<std::optional<state>> results(opt_.jobs);
  run_jobs(
      jobs,
      [&](Engine& we, int t) {
        results[t % opt_.jobs] = we.search_output(st, opt_.oneoutput);
      },
      [&](int first, int count) {
        for (int t = first; t < first + count; t++) {
          finish_iteration(t + 1, results[t % opt_.jobs], &st);
          results[t % opt_.jobs].reset();
        }
      });
}

static int count_state_outputs(const state& st) {
  int n = 0;
  for (int i = 0; i < 8; i++) {
    if (st.outputs[i] != NO_GATE) n += 1;
  }
  return n;
}

void Engine::generate_graph(const state& st_in) {
  // Multi-output beam search, keeping up to `beam` tied-minimum start
  // states per added output (parity: sboxgates.c:701-788). With
  // opt.jobs > 1 (single-process), the (start state x missing output)
  // searches of one iteration run as parallel independent jobs (engines
  // rotate over visible GPUs); bounds fold between iterations instead of
  // between tasks — slightly weaker mid-iteration pruning, same results
  // semantics.
  int num_start_states = 1;
  state start_states[20];
  start_states[0] = st_in;

  const bool parallel = opt_.jobs > 1 && ctx_->world() == 1;

  int num_outputs;
  while ((num_outputs = count_state_outputs(start_states[0])) < num_outputs_) {
    // Size of the states kept so far, and the bound of the searches to come.
    int best = opt_.metric == METRIC_GATES ? MAX_GATES : INT_MAX;
    state out_states[20];
    int num_out_states = 0;

    struct Task {
      int current;
      u8 output;
    };
    auto start_of = [&](const Task& task) {
      state st = start_states[task.current];
      set_metric_bound(st, opt_.metric, best);
      return st;
    };
    // Fold a search result into the beam.
    auto fold = [&](const Task& task, const std::optional<state>& st) {
      if (!st) {
        if (opt_.verbosity >= 0) {
          std::printf("No solution for output %d.\n", task.output);
        }
        return;
      }
      save_checkpoint(*st);
      if (best > metric_value(*st, opt_.metric)) {
        best = metric_value(*st, opt_.metric);
        num_out_states = 0;
      }
      if (metric_value(*st, opt_.metric) <= best) {
        if (num_out_states < std::min(20, opt_.beam)) {
          out_states[num_out_states++] = *st;
        } else if (opt_.verbosity >= 0) {
          std::printf("Output state buffer full! Throwing away valid state.\n");
        }
      }
    };

    for (int iter = 0; iter < opt_.iterations; iter++) {
      if (opt_.verbosity >= 0) {
        std::printf("Generating circuits with %d output%s. (%d/%d)\n", num_outputs + 1,
                    num_outputs == 0 ? "" : "s", iter + 1, opt_.iterations);
      }

      // Collect this iteration's tasks.
      std::vector<Task> tasks;
      for (int current = 0; current < num_start_states; current++) {
        for (u8 output = 0; output < num_outputs_; output++) {
          if (start_states[current].outputs[output] != NO_GATE) continue;
          tasks.push_back({current, output});
        }
      }

      if (!parallel) {
        for (const Task& task : tasks) {
          if (opt_.verbosity >= 0) {
            std::printf("Generating circuit for output %d...\n", task.output);
          }
          fold(task, search_output(start_of(task), task.output));
        }
      } else {
        // `best` stands still while the jobs run: one bound for the round.
        std::vector<Job> jobs;
        for (int ti = 0; ti < static_cast<int>(tasks.size()); ti++) {
          jobs.push_back({opt_.seed + 0x51ED * (iter * 1024 + ti + 1),
                          "beam job (state " + std::to_string(tasks[ti].current) +
                              ", output " + std::to_string(tasks[ti].output) + ")"});
        }
        std::vector<std::optional<state>> results(tasks.size());
        run_jobs(jobs, [&](Engine& we, int ti) {
          results[ti] = we.search_output(start_of(tasks[ti]), tasks[ti].output);
        });
        for (size_t ti = 0; ti < tasks.size(); ti++) fold(tasks[ti], results[ti]);
      }
    }
    if (num_out_states == 0) {
      // No output could be added within bounds; stop rather than loop
      // forever (the reference would loop with an empty beam).
      if (opt_.verbosity >= 0) std::printf("No solution found.\n");
      return;
    }
    if (opt_.verbosity >= 0) {
      if (opt_.metric == METRIC_GATES) {
        std::printf("Found %d state%s with %d gates.\n", num_out_states,
                    num_out_states == 1 ? "" : "s",
                    best - get_num_inputs(&out_states[0]));
      } else {
        std::printf("Found %d state%s with SAT metric %d.\n", num_out_states,
                    num_out_states == 1 ? "" : "s", best);
      }
    }
    for (int i = 0; i < num_out_states; i++) start_states[i] = out_states[i];
    num_start_states = num_out_states;
  }
}

}  // namespace sbg
