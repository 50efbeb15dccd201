// options.hpp — user-facing search configuration (flag-for-flag parity with
// the reference options struct, sboxgates.h:49-66, plus MI355X additions:
// seed control, GPU selection, output directory).
#pragma once

#include <string>

#include "sbg/boolfunc.hpp"
#include "sbg/state.hpp"

namespace sbg {

enum gpu_mode_t : i32 {
  GPU_AUTO = 0,   // use a GPU when one is visible
  GPU_OFF = 1,
  GPU_FORCE = 2,  // fail loudly if no GPU / kernels unavailable
};

// Where the pair sweeps of gate-mode steps 3 and 4a run on an engine that
// has a GPU. The circuit found is the same under all three: the pair scan
// reports the hit of the lowest rank, which is the host sweep's first match.
enum gpu_pairs_t : i32 {
  PAIRS_OFF = 0,    // host sweep
  PAIRS_AUTO = 1,   // GPU pair scan from GPU_PAIRS_MIN pairs upward
  PAIRS_FORCE = 2,  // GPU pair scan for every sweep
};

// PAIRS_AUTO cutover, in pairs C(n,2) of the node's pool: n = 170, the
// smallest measured pool at which the scan-service round trip of a k=2
// request (16.6 us per node) beat the host sweep of a node that misses
// (19.8 us; at n = 140 the host still won, 13.6 us against 16.6 us). Table
// and derivation: profiles/gate_mode_service.md.
constexpr i64 GPU_PAIRS_MIN = 170 * 169 / 2;

// CPU/GPU cutover of the shared-input two-LUT scan (options::lut_shared), in
// combinations C(n,4) of the window: C(21,4). A whole-range one-shot k_scan4s
// launch costs 32-90 us up to 28 gates; cpu_scan4s crosses it between 16 and
// 20 gates under a full mask (18.8 us against 32.2 us at 16 gates, 44.0 us
// against 32.6 us at 20) and between 20 and 28 gates under a sparse one
// (52 us against 90 us at 20, 338 us against 56 us at 28; interpolated about
// 6,000 combinations). The sparse crossing is the one taken: the nodes that
// reach this scan deep in the recursion carry sparse masks. Table:
// profiles/lut_shared_scan.md.
constexpr i64 GPU_SHARED_MIN = 21 * 20 * 19 * 18 / 24;

struct options {
  std::string fname;        // Input file (S-box table, or XML for -c/-d).
  std::string gfname;       // -g: initial graph file.
  int iterations = 1;       // -i
  int oneoutput = -1;       // -o
  int permute = 0;          // -p
  metric_t metric = METRIC_GATES;  // -s selects SAT
  bool output_c = false;    // -c
  bool output_dot = false;  // -d
  bool output_hip = false;  // --convert-hip (new: HIP device-function codegen)
  bool lut_graph = false;   // -l
  bool randomize = true;    // always on, as in the reference (sboxgates.c:1070)
  bool try_nots = false;    // -n
  int verbosity = 0;        // -v (counted)

  boolfunc avail_gates[17]; // terminated by num_inputs == 0
  boolfunc avail_not[49];
  boolfunc avail_3[257];
  int num_avail_3 = 0;

  // MI355X-native additions.
  bool seeded = false;      // --seed given: deterministic RNG
  u64 seed = 0;
  gpu_mode_t gpu = GPU_AUTO;
  gpu_pairs_t gpu_pairs = PAIRS_OFF;  // --gpu-pairs
  bool lut_shared = false;  // --lut-shared: LUT mode also tries two LUTs that
                            // share an input, LUT(LUT(x,y,z), d, s) with s
                            // one of x, y, z, before the 5-LUT scan
  bool ordered = false;     // --ordered: every GPU scan reports the hit of the
                            // lowest rank, i.e. what the CPU scan of the same
                            // window reports, so a seeded search finds the
                            // same circuit with and without a GPU. With more
                            // than one rank the result is reproducible for a
                            // fixed world and chunk size, not equal to the
                            // single-rank one. No effect without a GPU.
  int gpu_device = -1;      // HIP device index; -1 = current device
  int num_gpus = 1;         // CLI --gpus: in-process devices (threads)
  int beam = 20;            // --beam: tied-state beam width (<= 20; the
                            // reference hard-codes 20, sboxgates.c:704)
  int jobs = 1;             // --jobs: parallel independent search
                            // iterations (one engine per job; jobs rotate
                            // over visible GPUs)
  std::string output_dir;   // where XML checkpoints are written ("" = CWD)
  bool save_states = true;  // library callers may disable checkpoint writes

  // Fills avail_gates from a 16-bit gate-set bitfield (bit i = 2-input
  // function i available). Parity: sboxgates.c:870-880.
  void set_avail_gates(u32 bitfield) {
    int gatep = 0;
    for (int i = 0; i < 16; i++) {
      if (bitfield & (1u << i)) avail_gates[gatep++] = make_2_input_fun(static_cast<u8>(i));
    }
    avail_gates[gatep].num_inputs = 0;
  }

  // Derives avail_not / avail_3 from avail_gates. Call after set_avail_gates
  // and after try_nots is final (parity: sboxgates.c:974-981).
  void derive_function_lists() {
    int num = 0;
    if (try_nots) num = get_not_functions(avail_gates, avail_not);
    avail_not[num].num_inputs = 0;
    num_avail_3 = get_3_input_function_list(avail_gates, avail_3, try_nots);
    avail_3[num_avail_3].num_inputs = 0;
  }
};

// Default gate set: AND + OR + XOR (bitfield 194; sboxgates.c:1078).
constexpr u32 DEFAULT_GATE_BITFIELD = 2 + 64 + 128;

}  // namespace sbg
