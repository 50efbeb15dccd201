// scan5_geom.hpp — task geometry of k_scan5's wide walk, compiled by the
// kernel and by the host (bindings.cpp exposes it, so its arithmetic is
// tested without a GPU).
//
// A wide task is (triple, row d, word group): the pairs (d, e) with e among
// the GB gates of one group of the gate-transposed pool. Groups are aligned
// to the pool's END: inside the walk a gate has the shifted id
// s = gate + pad, pad = (GB - n % GB) % GB, so that the last gate sits on
// the top bit of a full group and the ids that no gate has (s < pad) are
// the low bits of group 0, the group with the fewest rows. Real ids appear
// only at the edges: the flat pair index, the exclusion set and what a
// survivor reports.
#pragma once

#include "sbg/gpu.hpp"
#include "sbg/ttable.hpp"

#if defined(__HIP__)
#define SBG_GEOM_FN __host__ __device__ __attribute__((always_inline)) inline
#else
#define SBG_GEOM_FN inline
#endif

namespace sbg {

constexpr int SCAN5_WIDE_GB = 32 * SCAN5_WIDE_WORDS;  // gates per task

SBG_GEOM_FN int scan5_wide_pad(int n) {
  return (SCAN5_WIDE_GB - n % SCAN5_WIDE_GB) % SCAN5_WIDE_GB;
}

// Word groups of the triple whose last gate is c, 0 <= c <= n - 3: group wg
// holds the shifted ids [GB wg, GB wg + GB) and has the rows
// c < d <= min(n - 2, GB wg + GB - 2 - pad). Only the last group is cut by
// n - 2; it has all m - 1 rows, m = n - 1 - c.
struct Scan5WideGroups {
  int w_min, w_max;  // first and last group that hold an e > c + 1
};
SBG_GEOM_FN Scan5WideGroups scan5_wide_groups(int n, int pad, int c) {
  constexpr int GB = SCAN5_WIDE_GB;
  return {(c + pad + 2) / GB, (n + pad - 1) / GB};
}

// Rows of group wg < w_max.
SBG_GEOM_FN int scan5_wide_rows(int pad, int c, int wg) {
  constexpr int GB = SCAN5_WIDE_GB;
  return GB * wg + GB - 2 - (c + pad);
}

// Tasks of the triple: the sum of its groups' rows.
SBG_GEOM_FN int scan5_wide_task_count(int n, int pad, int c) {
  constexpr int GB = SCAN5_WIDE_GB;
  const Scan5WideGroups g = scan5_wide_groups(n, pad, c);
  const int k = g.w_max - g.w_min;  // groups not cut by n - 2
  return (n - 2 - c) + k * (GB - 2 - (c + pad)) +
         GB * (k * (g.w_min + g.w_max - 1) / 2);
}

struct Scan5WideTask {
  int wg;  // word group: G words [NW wg, NW wg + NW)
  int d2;  // row inside the triple, d = c + 1 + d2
  int d;
  int e0;  // real id of the gate on bit 0; negative in group 0 when pad > 0
  int q0;  // flat pair index of bit 0 (of the pair (d, e0), which need not
           // exist): bit i is the pair with flat index q0 + i
};

// Task index -> task, 0 <= task < scan5_wide_task_count. Consecutive tasks
// take consecutive rows of one group, last group first (it has the most
// rows, so the search is short).
SBG_GEOM_FN Scan5WideTask scan5_wide_decode(int n, int pad, int c, int task) {
  constexpr int GB = SCAN5_WIDE_GB;
  const int m = n - 1 - c;
  Scan5WideTask t;
  t.wg = (n + pad - 1) / GB;
  t.d2 = task;
  for (int rows = m - 1; t.d2 >= rows; rows = scan5_wide_rows(pad, c, t.wg)) {
    t.d2 -= rows;
    t.wg--;
  }
  t.d = c + 1 + t.d2;
  t.e0 = GB * t.wg - pad;
  t.q0 = t.d2 * m - t.d2 * (t.d2 + 1) / 2 + t.e0 - t.d - 1;
  return t;
}

// The task's bits that are pairs to test: e > d, flat index inside the
// triple's window [lo, hi), neither gate in excl (real ids below 64). The
// group's top bit is at most gate n - 1, so the pool's end clips nothing.
SBG_GEOM_FN u64 scan5_wide_valid(const Scan5WideTask& t, int lo, int hi,
                                 u64 excl) {
  constexpr int GB = SCAN5_WIDE_GB;
  static_assert(GB == 32 || GB == 64);
  int i_lo = t.d + 1 - t.e0;
  if (i_lo < 0) i_lo = 0;
  if (i_lo < lo - t.q0) i_lo = lo - t.q0;
  int i_hi = GB;
  if (i_hi > hi - t.q0) i_hi = hi - t.q0;
  if (i_lo >= i_hi) return 0;
  u64 valid = (~0ULL >> (64 - i_hi)) & (~0ULL << i_lo);  // 1 <= i_hi <= 64
  if (excl != 0) {
    // An excluded d drops the whole row; excluded e's leave the mask with
    // one shift per task: bit i is gate e0 + i, and -64 < e0.
    if (t.d < 64 && ((excl >> t.d) & 1)) return 0;
    if (t.e0 < 0) {
      valid &= ~(excl << -t.e0);
    } else if (t.e0 < 64) {
      valid &= ~(excl >> t.e0);
    }
  }
  return valid;
}

}  // namespace sbg
