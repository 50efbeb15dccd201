// scan.hpp — candidate-scan primitives over a gate pool.
//
// Each scan walks a contiguous lexicographic range of k-combinations of the
// pool's gate truth tables and reports the first combination that admits a
// LUT (or LUT composition) realizing `target` under `mask`. The CPU
// implementations here are both the no-GPU execution path and the oracle
// for the CDNA4 kernels (gpu.hpp) in tests. Result layout matches the
// reference's res[10] wire format (lut.h:40-55):
//   3-LUT: res[0]=func,                res[1..3]=gate ids
//   5-LUT: res[0]=fo, res[1]=fi,       res[2..6]=gate ids (outer a,b,c; d,e)
//   7-LUT: res[0]=fo, res[1]=fm, res[2]=fi, res[3..9]=gate ids
// The shared-input two-LUT scan (SCAN_SHARED) reports in the 5-LUT layout,
// with res[6] equal to one of res[2..4].
// "First" is exact on the CPU: the scans walk in rank order, and the random
// word of a candidate is keyed on (seed, rank). The GPU kernels by default
// report whichever hit wins their election; a request with `ordered` set
// makes them report the hit of the lowest rank, with the CPU's result words.
// The pair scan (k=2, gate-mode steps 3 and 4a) always reports the hit of
// the lowest rank, on both sides, see cpu_scan2.
#pragma once

#include <vector>

#include "sbg/comb.hpp"
#include "sbg/common.hpp"
#include "sbg/state.hpp"
#include "sbg/ttable.hpp"

namespace sbg {

struct ScanResult {
  bool found = false;
  u16 res[10] = {};
  u64 evaluated = 0;  // combinations examined (for candidates/sec reporting)
};

// Precomputed matcher for the gate-mode step-4 triple scan: for every
// (care, req1) cell-requirement pair, whether some available composed
// 3-input function satisfies it. bitmap bit index = care*256 + req1.
// Built once per option set from avail_3 (8.2 KB; O(256^2 * |avail|) host
// preprocessing turns the reference's per-candidate 256-function x 4-order
// truth-table loop, sboxgates.c:406-432, into one bit probe per argument
// order).
struct Avail3Matcher {
  u8 bitmap[256 * 256 / 8];
  u8 funs[256];     // available function bytes, search order
  u8 cost[256];     // gates added when realized (1 + #input NOTs + not_out)
  int count;
};

// Precomputed matcher for the pair scan (k=2) over one 2-input function
// list: entry[care << 4 | req1] is m | swapped << 7 for the first function m
// of the list, in list order, that meets the 4-cell requirements directly
// or, when it is not ab_commutative, with its arguments swapped (direct
// before swapped, both before m + 1). PAIR2_NONE: no function does. A list
// holds at most 48 entries.
constexpr u8 PAIR2_NONE = 0xFF;
struct Pair2Matcher {
  u8 entry[256];
};

// Packed scan request shared by CPU and GPU paths.
struct ScanRequest {
  const ttable* tables;  // gate pool truth tables, ids 0..n-1
  int n;                 // pool size (state.num_gates)
  ttable target;
  ttable mask;
  u64 excl_low64;        // bitmask of excluded gate ids < 64 (the inbits)
  u64 seed;              // randomization source
  bool count_all;        // true: never early-exit (bench mode)
  const Avail3Matcher* matcher = nullptr;  // k=4 scans only
  const Pair2Matcher* matcher2 = nullptr;  // k=2 scans only
  // k=2 scans only: visit position j holds gate order[j], a permutation of
  // the pool ids; null is the identity.
  const gatenum* order = nullptr;
  // GPU scans only (options::ordered): report the hit of the lowest rank in
  // the window, which is what the CPU scan of that window returns, res[10]
  // word for word, instead of whichever hit wins the election. The CPU
  // scans walk in rank order and need no flag; count_all ignores it.
  bool ordered = false;
};

// Exclusion mask of a request from the multiplexer input bits already used
// on the path to this node (a list of at most 8 ended by -1).
inline u64 excl_from_inbits(const i8* inbits) {
  u64 excl = 0;
  for (int i = 0; i < 8 && inbits[i] != -1; i++) {
    if (inbits[i] < 64) excl |= 1ULL << inbits[i];
  }
  return excl;
}

// The request for a scan over all of st's gates. Their truth tables go into
// `pool`, which the caller keeps alive while the request is in use.
inline ScanRequest make_scan_request(std::vector<ttable>& pool, const state& st,
                                     const ttable& target, const ttable& mask,
                                     u64 seed, u64 excl = 0,
                                     const Avail3Matcher* matcher = nullptr) {
  pool.resize(st.num_gates);
  for (int i = 0; i < st.num_gates; i++) pool[i] = st.gates[i].table;
  return ScanRequest{.tables = pool.data(), .n = st.num_gates, .target = target,
                     .mask = mask, .excl_low64 = excl, .seed = seed,
                     .count_all = false, .matcher = matcher};
}

// 3-LUT: scan combinations [begin, end) of C(n,3).
ScanResult cpu_scan3(const ScanRequest& rq, i64 begin, i64 end);

// 5-LUT: scan combinations [begin, end) of C(n,5).
ScanResult cpu_scan5(const ScanRequest& rq, i64 begin, i64 end);

// Scan kind of the shared-input two-LUT scan for Engine::scan and
// GpuEngine::scan. Not 4: that is the gate-mode triple scan.
constexpr int SCAN_SHARED = 40;

// Size of the combination space a scan kind ranks: C(n,3) for the gate-mode
// triple scan, C(n,4) for the shared-input scan, else C(n,k).
inline i64 scan_space(int n, int k) {
  return n_choose_k(n, k == 4 ? 3 : (k == SCAN_SHARED ? 4 : k));
}

// Shared-input two-LUT scan: combinations [begin, end) of C(n,4), each
// tried as LUT(LUT(x,y,z), d, s) with s one of x, y, z in the 12 shapes of
// lut4s_solve_from_p. Result in the 5-LUT layout: res[0]=fo, res[1]=fi,
// res[2..4]=outer triple (ascending), res[5]=rest gate d, res[6]=shared gate
// (one of res[2..4]). Honours excl_low64 and count_all as cpu_scan5 does.
ScanResult cpu_scan4s(const ScanRequest& rq, i64 begin, i64 end);

// 7-LUT: scan combinations [begin, end) of C(n,7); feasibility filter and
// (3,3,1) function assignment are fused per-range (no global frontier cap,
// unlike the reference's 100k-per-rank truncation, lut.c:291-318).
ScanResult cpu_scan7(const ScanRequest& rq, i64 begin, i64 end);

// Gate-mode step-4 triple scan (k=4): find a triple realized by an
// available composed 3-input function in one of the 6 argument orders.
// Result: res[0]=avail index, res[1]=argument order (TRIPLE_PERMS index),
// res[2..4]=gate ids. Requires rq.matcher.
ScanResult cpu_scan4(const ScanRequest& rq, i64 begin, i64 end);

// Pair scan (k=2): walks ranks [begin, end) of C(n,2), row-major over visit
// positions i < k, and reports the hit of the LOWEST rank in the window
// (deterministic, unlike the other scans). With x = order[i], y = order[k]:
// a pair whose 4-cell requirements under (target, mask) are contradictory
// misses, otherwise rq.matcher2 names the function. res[0]=index into the
// function list, res[1]=1 if the arguments are swapped, res[2..3]=gate ids
// in argument order (what add_boolfunc_2 takes). evaluated = hit rank -
// begin + 1, or the window's size on a miss. excl_low64, seed and count_all
// have no effect. Requires rq.matcher2.
ScanResult cpu_scan2(const ScanRequest& rq, i64 begin, i64 end);

// Builds the pair matcher of a 2-input function list ended by
// num_inputs == 0.
void build_pair2_matcher(const boolfunc* funs, Pair2Matcher* out);

// The pair scan's result from its packed minimum `best` = hit rank << 8 |
// matcher entry, all-ones when nothing hit. [begin, end) already clipped.
ScanResult pair2_result(u64 best, const ScanRequest& rq, i64 begin, i64 end);

// Pattern-space table of a 2-input function: bit p = value at pattern
// p = a << 1 | b (the 4-bit encoding is bit-reversed; see boolfunc.hpp).
inline u8 fun2_pattern_table(u8 fun) {
  u8 out = 0;
  for (u8 p = 0; p < 4; p++) out |= static_cast<u8>(fun2_val(fun, p) << p);
  return out;
}

// Swaps the two input roles of a 4-bit pattern mask (pattern a << 1 | b ->
// b << 1 | a): bits 1 and 2 exchange.
inline u8 swap_pair_patterns(u8 m) {
  return static_cast<u8>((m & 0x9) | ((m & 2) << 1) | ((m & 4) >> 1));
}

// Builds the matcher from an avail_3-style list (funs/cost arrays).
void build_avail3_matcher(const u8* funs, const u8* costs, int count,
                          Avail3Matcher* out);

// The 6 argument orders for a triple; shared by host and device code.
// TRIPLE_PERMS[p] selects which canonical input feeds A, B, C.
extern const int TRIPLE_PERMS6[6][3];

// Permute an 8-bit cell mask: out bit (v[s0]<<2|v[s1]<<1|v[s2]) = in bit
// (v0<<2|v1<<1|v2).
u8 permute_cells8_host(u8 m, const int* sel);

// --- Naive reference-style checkers (test oracles; see lut.c:34-109) ---

// True if some k-input LUT over `tables` can realize target under mask.
bool naive_check_n_lut_possible(int num, const ttable& target, const ttable& mask,
                                const ttable* tables);

// Derives a 3-LUT function by per-position constraint propagation.
bool naive_get_lut_function(const ttable& a, const ttable& b, const ttable& c,
                            const ttable& target, const ttable& mask, u8* func);

}  // namespace sbg
