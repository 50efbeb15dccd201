// scan5_cell.hpp — what k_scan5_wave works out once per triple before it
// walks the triple's pairs, compiled by the kernel and by the host
// (bindings.cpp exposes it, so its rules are tested without a GPU). In the
// kernel one lane runs this for one triple of a chunk, so nothing here
// crosses lanes or touches memory: truth tables come as eight 32-bit
// dwords, dword w holding the table positions [32 w, 32 w + 32).
//
// The triple (a, b, c) splits the table positions into eight prefix cells:
// position p lies in cell u = ta[p] << 2 | tb[p] << 1 | tc[p]. A cell's two
// sides are its positions where the target is forced to 1 (T1) and to 0
// (T0). A cell is live if both sides are non-empty: only a live cell can
// contradict a candidate. The screen runs on the live cell whose smaller
// side is largest, ties to the lower cell, and on cell 7 when none is live
// (an empty side rejects nothing, so everything passes the screen then).
#pragma once

#include "sbg/scan5_geom.hpp"

namespace sbg {

// Dword of prefix cell u: the positions with (ta, tb, tc) == u's bits.
SBG_GEOM_FN u32 scan5_cell_dword(u32 ra, u32 rb, u32 rc, int u) {
  return ((u & 4) ? ra : ~ra) & ((u & 2) ? rb : ~rb) & ((u & 1) ? rc : ~rc);
}

struct Scan5ScreenCell {
  u32 live;  // bit u: cell u is live
  int u0;    // the screen cell
  int c1;    // positions of the screen cell's target-1 side (at most 256)
  int c0;    // ... and of its target-0 side
};

SBG_GEOM_FN Scan5ScreenCell scan5_screen_cell(const u32 (&ra)[8],
                                              const u32 (&rb)[8],
                                              const u32 (&rc)[8],
                                              const u32 (&T1)[8],
                                              const u32 (&T0)[8]) {
  int n1[8] = {}, n0[8] = {};
#pragma unroll
  for (int w = 0; w < 8; w++) {
#pragma unroll
    for (int u = 0; u < 8; u++) {
      const u32 cell = scan5_cell_dword(ra[w], rb[w], rc[w], u);
      n1[u] += __builtin_popcount(cell & T1[w]);
      n0[u] += __builtin_popcount(cell & T0[w]);
    }
  }
  Scan5ScreenCell s;
  s.live = 0;
  s.c1 = n1[7];
  s.c0 = n0[7];
  // Largest (smaller side << 3 | 7 - u) over the live cells: the batch
  // kernel's rule. 0 stands for "none live" and names cell 7.
  u32 best = 0;
#pragma unroll
  for (int u = 0; u < 8; u++) {
    if (n1[u] == 0 || n0[u] == 0) continue;
    s.live |= 1u << u;
    const u32 key = (static_cast<u32>(n1[u] < n0[u] ? n1[u] : n0[u]) << 3) |
                    static_cast<u32>(7 - u);
    if (key > best) {
      best = key;
      s.c1 = n1[u];
      s.c0 = n0[u];
    }
  }
  s.u0 = 7 - static_cast<int>(best & 7u);
  return s;
}

// The first SCAN5_HEAD_BYTES positions of one side of a cell (h: the side's
// eight dwords), ascending, one per byte, byte 0 of head[0] first. A side
// with fewer positions repeats its last one in the remaining bytes
// (accumulating a position twice changes nothing); an empty side gives
// zeros, which nobody reads. These are the bytes that gt_build_lists files
// at the start of the side's list.
constexpr int SCAN5_HEAD_BYTES = 16;

SBG_GEOM_FN void scan5_side_head(const u32 (&h)[8], u32 (&head)[4]) {
  u32 x0 = 0, x1 = 0, x2 = 0, x3 = 0, p = 0;
  int cnt = 0;
  // The head is a 16-byte shift register: a new position enters at the top
  // byte, so after 16 pushes the first one sits in byte 0.
  const auto push = [&]() {
    x0 = (x0 >> 8) | (x1 << 24);
    x1 = (x1 >> 8) | (x2 << 24);
    x2 = (x2 >> 8) | (x3 << 24);
    x3 = (x3 >> 8) | (p << 24);
    cnt++;
  };
#pragma unroll
  for (int w = 0; w < 8; w++) {
    for (u32 m = h[w]; m != 0 && cnt < SCAN5_HEAD_BYTES; m &= m - 1) {
      p = static_cast<u32>(32 * w + __builtin_ctz(m));
      push();
    }
  }
  while (cnt < SCAN5_HEAD_BYTES) push();
  head[0] = x0;
  head[1] = x1;
  head[2] = x2;
  head[3] = x3;
}

}  // namespace sbg
