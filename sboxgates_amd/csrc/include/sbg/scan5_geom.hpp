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

// The task of row d2 in group wg, for a walk that keeps (wg, d2) itself
// (scan5_wide_decode finds them from a task index).
SBG_GEOM_FN Scan5WideTask scan5_wide_task_at(int n, int pad, int c, int wg,
                                             int d2) {
  constexpr int GB = SCAN5_WIDE_GB;
  const int m = n - 1 - c;
  Scan5WideTask t;
  t.wg = wg;
  t.d2 = d2;
  t.d = c + 1 + d2;
  t.e0 = GB * wg - pad;
  t.q0 = d2 * m - d2 * (d2 + 1) / 2 + t.e0 - t.d - 1;
  return t;
}

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

// ---------------------------------------------------------------------------
// Chunks of k_scan5_wave's triple queue. A wave takes a whole chunk of
// consecutive triples with one atomic on a chunk counter; chunk k of a queue
// of `units` triples that `waves` waves share is [first, first + count),
// relative to the queue's first triple. The bulk comes in chunks of `size`
// triples: at most SCAN5_CHUNK_MAX (one triple per lane of the wave that
// decodes the chunk), few enough that every wave still gets
// SCAN5_CHUNKS_PER_WAVE of them, and at least SCAN5_CHUNK_MIN, because one
// address serves only about one agent-scope atomic per 12 ns: a scan with
// few triples must not pay one per triple (the host sizes its grid to a
// chunk of SCAN5_CHUNK_MIN per wave). The end of the queue is handed out in
// `waves` chunks of each smaller size size / 2, size / 4, ..., down to
// SCAN5_CHUNK_MIN, so the waves finish close together.
// ---------------------------------------------------------------------------
constexpr int SCAN5_CHUNK_MAX = 64;
constexpr int SCAN5_CHUNK_MIN = 8;
constexpr int SCAN5_CHUNKS_PER_WAVE = 8;

SBG_GEOM_FN int scan5_chunk_size(i64 units, int waves) {
  const i64 s = units / (static_cast<i64>(SCAN5_CHUNKS_PER_WAVE) * waves);
  return s < SCAN5_CHUNK_MIN
             ? SCAN5_CHUNK_MIN
             : (s > SCAN5_CHUNK_MAX ? SCAN5_CHUNK_MAX : static_cast<int>(s));
}

// What does not depend on k, worked out once per wave (the divisions).
struct Scan5ChunkPlan {
  i64 units;
  int waves;
  int size;   // triples per bulk chunk
  i64 bulk;   // triples handed out in bulk chunks
  i64 nbulk;  // bulk chunks; the last one may be short
};

SBG_GEOM_FN Scan5ChunkPlan scan5_chunk_plan(i64 units, int waves) {
  Scan5ChunkPlan p;
  p.units = units < 0 ? 0 : units;
  p.waves = waves;
  p.size = scan5_chunk_size(p.units, waves);
  i64 tail = 0;  // size > CHUNK_MIN implies units >= 8 waves size > tail
  for (int s = p.size / 2; s >= SCAN5_CHUNK_MIN; s /= 2) {
    tail += static_cast<i64>(waves) * s;
  }
  p.bulk = p.units - tail;
  p.nbulk = (p.bulk + p.size - 1) / p.size;
  return p;
}

struct Scan5Chunk {
  i64 first;
  int count;  // 0: k is past the last chunk
};

SBG_GEOM_FN Scan5Chunk scan5_chunk(const Scan5ChunkPlan& p, i64 k) {
  if (k < p.nbulk) {
    const i64 first = k * p.size;
    const i64 left = p.bulk - first;
    return {first, left < p.size ? static_cast<int>(left) : p.size};
  }
  k -= p.nbulk;
  i64 first = p.bulk;
  for (int s = p.size / 2; s >= SCAN5_CHUNK_MIN; s /= 2) {
    if (k < p.waves) return {first + k * s, s};
    k -= p.waves;
    first += static_cast<i64>(p.waves) * s;
  }
  return {p.units, 0};
}

}  // namespace sbg
