"""The per-triple set-up rules of k_scan5_wave (sbg/scan5_cell.hpp, the code
the kernel compiles), against a few lines of plain Python: which prefix
cells are live, which one the screen runs on, and the first 16 positions of
a side. No GPU.

The rule: position p lies in prefix cell u = ta[p] << 2 | tb[p] << 1 | tc[p].
A cell's sides are its positions inside T1 and inside T0. A cell is live if
both sides are non-empty. The screen cell is the live cell whose smaller
side is largest, ties to the lower cell, and cell 7 when none is live.
"""

import random

import pytest

from sboxgates_amd import _core

ALL = (1 << 256) - 1


def tb(value):
    return value.to_bytes(32, "little")


def cell_of(ta, tb_, tc, u):
    m = ALL
    for bit, t in ((4, ta), (2, tb_), (1, tc)):
        m &= t if u & bit else ~t & ALL
    return m


def rule(ta, tb_, tc, T1, T0):
    """(live, u0, size of u0's T1 side, size of u0's T0 side)."""
    sizes = [(bin(cell_of(ta, tb_, tc, u) & T1).count("1"),
              bin(cell_of(ta, tb_, tc, u) & T0).count("1")) for u in range(8)]
    live = [u for u in range(8) if sizes[u][0] and sizes[u][1]]
    u0 = 7
    if live:
        top = max(min(sizes[u]) for u in live)
        u0 = min(u for u in live if min(sizes[u]) == top)
    return sum(1 << u for u in live), u0, sizes[u0][0], sizes[u0][1]


def check(ta, tb_, tc, T1, T0):
    want = rule(ta, tb_, tc, T1, T0)
    got = _core.scan5_screen_cell(tb(ta), tb(tb_), tb(tc), tb(T1), tb(T0))
    assert tuple(got) == want, (hex(ta), hex(tb_), hex(tc), hex(T1), hex(T0))
    return want


def tables_for(cells):
    """ta, tb, tc that put position p into cell cells[p]."""
    ta = sum(1 << p for p, u in enumerate(cells) if u & 4)
    tb_ = sum(1 << p for p, u in enumerate(cells) if u & 2)
    tc = sum(1 << p for p, u in enumerate(cells) if u & 1)
    return ta, tb_, tc


@pytest.mark.parametrize("seed", range(40))
def test_random_tables_and_masks(seed):
    rng = random.Random(seed)
    ta, tb_, tc, target = (rng.getrandbits(256) for _ in range(4))
    # Full mask, and sparse masks of 2 to 64 positions.
    for size in (256, 64, 17, 8, 3, 2):
        mask = sum(1 << p for p in rng.sample(range(256), size))
        check(ta, tb_, tc, target & mask, ~target & mask & ALL)


@pytest.mark.parametrize("seed", range(10))
def test_cell_positions(seed):
    rng = random.Random(100 + seed)
    ta, tb_, tc = (rng.getrandbits(256) for _ in range(3))
    got = [int.from_bytes(_core.scan5_cell(tb(ta), tb(tb_), tb(tc), u),
                          "little") for u in range(8)]
    assert got == [cell_of(ta, tb_, tc, u) for u in range(8)]
    assert sum(got) == ALL  # the cells partition the positions


def test_no_live_cell():
    rng = random.Random(5)
    cells = [rng.randrange(8) for _ in range(256)]
    ta, tb_, tc = tables_for(cells)
    # Cells 0..3 hold only target-1 positions, cells 4..7 only target-0.
    T1 = sum(1 << p for p, u in enumerate(cells) if u < 4)
    live, u0, c1, c0 = check(ta, tb_, tc, T1, ALL & ~T1)
    assert (live, u0) == (0, 7) and c1 == 0


def test_empty_sides():
    rng = random.Random(6)
    ta, tb_, tc, T = (rng.getrandbits(256) for _ in range(4))
    assert check(ta, tb_, tc, 0, T)[:2] == (0, 7)
    assert check(ta, tb_, tc, T, 0)[:2] == (0, 7)
    assert check(ta, tb_, tc, 0, 0) == (0, 7, 0, 0)


@pytest.mark.parametrize("u", range(8))
def test_exactly_one_live_cell(u):
    rng = random.Random(7 + u)
    cells = [rng.randrange(8) for _ in range(256)]
    ta, tb_, tc = tables_for(cells)
    inside = [p for p, c in enumerate(cells) if c == u]
    # Everything outside cell u is target-1; cell u has one target-0 position.
    T0 = 1 << inside[0]
    live, u0, c1, c0 = check(ta, tb_, tc, ALL & ~T0, T0)
    assert (live, u0, c0) == (1 << u, u, 1) and c1 == len(inside) - 1


def test_ties_go_to_the_lower_cell():
    # Cells 2, 5 and 6 each have a smaller side of 3; cell 1 has 2; cell 7
    # has sides of 40 and 0 (not live).
    cells, T1, p = [], 0, 0
    for u, n1, n0 in ((2, 3, 9), (5, 7, 3), (6, 3, 3), (1, 2, 30), (7, 40, 0)):
        for k in range(n1 + n0):
            cells.append(u)
            if k < n1:
                T1 |= 1 << p
            p += 1
    used = p
    cells += [0] * (256 - used)  # cell 0: outside both T1 and T0
    ta, tb_, tc = tables_for(cells)
    T0 = ((1 << used) - 1) & ~T1
    assert check(ta, tb_, tc, T1, T0) == (0b01100110, 2, 3, 9)
    # Cell 2 loses a position on its smaller side: 5 and 6 tie, 5 wins.
    first = cells.index(2)
    assert check(ta, tb_, tc, T1 & ~(1 << first), T0) == (0b01100110, 5, 7, 3)


def test_side_of_256_positions():
    # One cell holds every position; all of them target-1: not live.
    assert check(ALL, 0, ALL, ALL, 0) == (0, 7, 0, 0)
    assert check(ALL, 0, ALL, 0, ALL) == (0, 7, 0, 0)
    # 255 against 1, and the sizes come back unclipped.
    assert check(ALL, 0, ALL, ALL & ~(1 << 200), 1 << 200) == (1 << 5, 5, 255, 1)
    assert check(0, 0, 0, 1, ALL & ~1) == (1, 0, 1, 255)


def head_rule(side):
    pos = [p for p in range(256) if (side >> p) & 1][:_core.SCAN5_HEAD_BYTES]
    if not pos:
        return None
    return pos + [pos[-1]] * (_core.SCAN5_HEAD_BYTES - len(pos))


@pytest.mark.parametrize("size", [1, 2, 3, 4, 5, 15, 16, 17, 33, 100, 256])
def test_side_head(size):
    rng = random.Random(size)
    for _ in range(20):
        side = sum(1 << p for p in rng.sample(range(256), size))
        assert _core.scan5_side_head(tb(side)) == head_rule(side)


def test_side_head_word_edges():
    for pos in ([0], [255], [31, 32], [63, 64, 127, 128, 191, 192, 255],
                list(range(224, 256)), list(range(0, 256, 16)),
                list(range(15, 256, 16))):
        side = sum(1 << p for p in pos)
        assert _core.scan5_side_head(tb(side)) == head_rule(side)
