"""k_scan5 wide walk (gfx950) against cpu_scan5 and the independent oracle.

Batches of triples whose longest row exceeds _core.SCAN5_WIDE_MIN_ROW screen
a row's e's a whole word group of the gate-transposed pool at a time: the
valid mask of a task is clipped to e > d, to the pool's end and to the
triple's window, excluded e's below 64 leave it with one shift, and what
passes keeps its flat rank. These tests aim at that arithmetic: gate ids on
both sides of every 32-gate word boundary, windows that end at and next to
such candidates, exclusion sets on the word edges, masks with few, one or no
live position, and the two pool sizes next to the crossover.

Pool 70 is the smallest with gate ids >= 64; pool 97 adds a fourth word.
"""

import functools
import math
import random

import pytest

import _oracle as orc
from sboxgates_amd import _core
from sboxgates_amd.ops import gen_lut_ttable, mask_for_inputs

pytestmark = pytest.mark.gpu

FULL = mask_for_inputs(8)
SEED = 11
WIDE_MIN_ROW = _core.SCAN5_WIDE_MIN_ROW
POOLS = (70, 97)


def assert_wide(n):
    """The pool's longest row (the gates behind triple (0, 1, 2)) takes the
    wide walk."""
    assert n - 3 > WIDE_MIN_ROW, (n, WIDE_MIN_ROW)


@pytest.fixture(scope="module")
def engines():
    if not _core.gpu_available():
        pytest.skip("no GPU")
    gpu, cpu = orc.make_pair(True)
    assert gpu.gpu_active
    return gpu, cpu


@functools.lru_cache(maxsize=None)
def pool(n):
    """(state, tables as bytes, tables as ints) of the pool with n gates."""
    st = orc.cpu_engine(5).initial_state()
    st.grow_pool_random(n, 0x1DE + n)
    assert st.num_gates == n
    tabs = [st.gate(i)["table"] for i in range(n)]
    return st, tabs, [orc.tt_int(t) for t in tabs]


@functools.lru_cache(maxsize=None)
def aes_target():
    return orc.cpu_engine(5).target(0)


def plant(tabs, ids, rng):
    """A non-constant target that LUT(LUT(a, b, c), d, e) over the gates
    `ids` realises, composed as in test_scan5_rows.plant."""
    full = orc.tt_int(FULL)
    for _ in range(100):
        t_o = gen_lut_ttable(rng.randrange(1, 255), tabs[ids[0]], tabs[ids[1]],
                             tabs[ids[2]])
        target = gen_lut_ttable(rng.randrange(1, 255), t_o, tabs[ids[3]],
                                tabs[ids[4]])
        if 0 < orc.tt_int(target) & full < full:
            return target
    raise AssertionError("no non-constant planted target")


@functools.lru_cache(maxsize=None)
def boundary_combs(n):
    """Triples (0,1,2) and (30,31,32) with d and e on both sides of the
    32-gate word boundaries, at the row's start and at the pool's end."""
    out = []
    for a, b, c in ((0, 1, 2), (30, 31, 32)):
        for d in sorted({c + 1, 30, 31, 32, 62, 63, 64}):
            if d <= c or d > n - 2:
                continue
            for e in sorted({d + 1, 31, 32, 33, 63, 64, 65, n - 1}):
                if d < e < n:
                    out.append((a, b, c, d, e))
    assert len(out) > 40
    return tuple(out)


@functools.lru_cache(maxsize=None)
def boundary_ranks(n):
    return tuple(orc.checked_rank(comb, n) for comb in boundary_combs(n))


def count_both(gpu, cpu, st, b, e, excl=0, target=None, mask=FULL):
    target = aes_target() if target is None else target
    _, _, ev_g = gpu.scan_pool(5, st, target, mask, b, e, seed=SEED,
                               count_all=True, excl=excl)
    _, _, ev_c = cpu.scan_pool(5, st, target, mask, b, e, seed=SEED,
                               count_all=True, excl=excl)
    return ev_g, ev_c


# ---------------------------------------------------------------------------
# 1. Verdicts at the word boundaries.
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", POOLS)
def test_word_boundary_verdicts(engines, n):
    """Single-rank windows on every boundary pair, checked both ways: with
    a target planted on the combination (found, valid, res as the CPU's) and
    with the plain AES bit-0 target (verdict as the oracle's and the CPU's).
    """
    assert_wide(n)
    gpu, cpu = engines
    st, tabs, ints = pool(n)
    rng = random.Random(0xB0 + n)
    aes = aes_target()
    t_int, m_int = orc.tt_int(aes), orc.tt_int(FULL)
    for comb, r in zip(boundary_combs(n), boundary_ranks(n)):
        assert orc.checked_unrank(r, n, 5) == list(comb)
        target = plant(tabs, comb, rng)
        f_g, r_g, ev_g = gpu.scan_pool(5, st, target, FULL, r, r + 1, seed=SEED)
        f_c, r_c, ev_c = cpu.scan_pool(5, st, target, FULL, r, r + 1, seed=SEED)
        assert f_c and f_g, (comb, f_g, f_c)
        assert ev_g == 1 and ev_c == 1, (comb, ev_g, ev_c)
        assert orc.hit_ids(5, r_g) == list(comb), (comb, list(r_g))
        orc.assert_hit_valid(5, st, r_g, target, FULL)
        assert list(r_g) == list(r_c), (comb, list(r_g), list(r_c))

        f_g, r_g, ev_g = gpu.scan_pool(5, st, aes, FULL, r, r + 1, seed=SEED)
        f_c, _, _ = cpu.scan_pool(5, st, aes, FULL, r, r + 1, seed=SEED)
        verdict = orc.found5([ints[i] for i in comb], t_int, m_int)
        assert ev_g == 1, (comb, ev_g)
        assert f_g == verdict, (comb, f_g, verdict)
        assert f_g == f_c, (comb, f_g, f_c)
        if f_g:
            orc.assert_hit_valid(5, st, r_g, aes, FULL)


# ---------------------------------------------------------------------------
# 2. Window clipping.
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", POOLS)
def test_window_clipping(engines, n):
    """count_all windows that begin or end at a boundary rank or next to it,
    200 random windows and the full range."""
    assert_wide(n)
    gpu, cpu = engines
    st, _, _ = pool(n)
    total = math.comb(n, 5)
    span = 3000
    windows = []
    for r in boundary_ranks(n):
        for x in (r - 1, r, r + 1):
            if 0 <= x < total:
                windows.append((x, min(total, x + span)))
            if 0 < x <= total:
                windows.append((max(0, x - span), x))
    rng = random.Random(0xC11 + n)
    for _ in range(200):
        length = int(2 ** rng.uniform(0, 17))
        b = rng.randrange(total - length)
        windows.append((b, b + length))
    for b, e in windows:
        ev_g, ev_c = count_both(gpu, cpu, st, b, e)
        assert ev_g == e - b, (b, e, ev_g)
        assert ev_g == ev_c, (b, e, ev_g, ev_c)
    _, _, ev = gpu.scan_pool(5, st, aes_target(), FULL, 0, total, seed=SEED,
                             count_all=True)
    assert ev == total


# ---------------------------------------------------------------------------
# 3. Exclusion at pool 70.
# ---------------------------------------------------------------------------
def bits(ids):
    out = 0
    for i in ids:
        assert i < 64
        out |= 1 << i
    return out


# Name -> (excluded ids, first gate id a window's combinations may start
# with). "absent" excludes only gates that no scanned combination holds.
EXCL_CASES = {
    "word_edges": ((31, 32, 63), 0),
    "row_d": ((40,), 0),
    "edges_and_d": ((31, 32, 40, 63), 0),
    "absent": ((0, 1, 2), 3),
}


@pytest.mark.parametrize("which", sorted(EXCL_CASES))
def test_exclusion_counts(engines, which):
    n = 70
    assert_wide(n)
    gpu, cpu = engines
    st, _, _ = pool(n)
    ids, first_a = EXCL_CASES[which]
    excl = bits(ids)
    total = math.comb(n, 5)
    # Ranks whose combination starts at first_a or later.
    lo = total - math.comb(n - first_a, 5)
    assert orc.unrank(lo, n, 5)[0] == first_a

    ev_g, ev_c = count_both(gpu, cpu, st, lo, total, excl=excl)
    assert ev_g == ev_c, (which, ev_g, ev_c)
    if first_a == 0:
        assert ev_g == math.comb(n - len(ids), 5)
    else:
        assert ev_g == total - lo
    rng = random.Random(excl & 0xFFFF)
    for _ in range(50):
        length = int(2 ** rng.uniform(0, 17))
        b = rng.randrange(lo, total - length)
        ev_g, ev_c = count_both(gpu, cpu, st, b, b + length, excl=excl)
        assert ev_g == ev_c, (which, b, length, ev_g, ev_c)
        if first_a != 0:
            assert ev_g == length, (which, b, length, ev_g)


# ---------------------------------------------------------------------------
# 4. A planted hit inside a wide window.
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", POOLS)
def test_planted_hit_in_window(engines, n):
    assert_wide(n)
    gpu, _ = engines
    st, tabs, _ = pool(n)
    total = math.comb(n, 5)
    rng = random.Random(0x91A + n)
    for comb, r in zip(boundary_combs(n), boundary_ranks(n)):
        target = plant(tabs, comb, rng)
        b, e = max(0, r - 2000), min(total, r + 2001)
        f_g, r_g, _ = gpu.scan_pool(5, st, target, FULL, b, e, seed=SEED)
        assert f_g, (comb, b, e)
        orc.assert_hit_valid(5, st, r_g, target, FULL)
        assert b <= orc.checked_rank(orc.hit_ids(5, r_g), n) < e, (comb, r_g)


# ---------------------------------------------------------------------------
# 5. Sparse and degenerate masks at pool 70.
# ---------------------------------------------------------------------------
def check_ranks(gpu, cpu, st, ints, n, target, mask, ranks):
    t_int, m_int = orc.tt_int(target), orc.tt_int(mask)
    hits = 0
    for r in ranks:
        comb = orc.checked_unrank(r, n, 5)
        f_g, r_g, ev_g = gpu.scan_pool(5, st, target, mask, r, r + 1, seed=SEED)
        f_c, r_c, _ = cpu.scan_pool(5, st, target, mask, r, r + 1, seed=SEED)
        verdict = orc.found5([ints[i] for i in comb], t_int, m_int)
        assert ev_g == 1, (r, ev_g)
        assert f_g == verdict, (r, comb, f_g, verdict)
        assert f_g == f_c, (r, comb, f_g, f_c)
        if f_g:
            hits += 1
            assert orc.hit_ids(5, r_g) == comb, (r, list(r_g))
            orc.assert_hit_valid(5, st, r_g, target, mask)
            assert list(r_g) == list(r_c), (r, list(r_g), list(r_c))
    return hits


def test_sparse_mask_verdicts(engines):
    """12 masked positions: the screen cell holds one or two of them."""
    n = 70
    assert_wide(n)
    gpu, cpu = engines
    st, _, ints = pool(n)
    target = aes_target()
    mask = orc.sparse_mask(0x5A12, 12, target)
    rng = random.Random(0x5A12)
    ranks = rng.sample(range(math.comb(n, 5)), 300)
    hits = check_ranks(gpu, cpu, st, ints, n, target, mask, ranks)
    print("sparse mask: hits in 300 ranks:", hits)


def ones_mask(target, count, seed):
    """`count` positions, all of them target-1: no cell of any triple has a
    forced-0 side, so no cell is live and the screen passes everything."""
    ones = orc.positions(orc.tt_int(target))
    m = 0
    for p in random.Random(seed).sample(ones, count):
        m |= 1 << p
    return orc.tt_bytes(m)


@pytest.mark.parametrize("count", [6, 1])
def test_no_live_cell(engines, count):
    """Every candidate survives the screen and goes to the solver: a
    2000-rank window gives what the CPU gives, and single ranks agree with
    the oracle."""
    n = 70
    assert_wide(n)
    gpu, cpu = engines
    st, _, ints = pool(n)
    target = aes_target()
    mask = ones_mask(target, count, 0x0E5 + count)
    orc.assert_mask_has_target1(target, mask)
    total = math.comb(n, 5)
    rng = random.Random(0x11FE + count)
    b = rng.randrange(total - 2000)
    ev_g, ev_c = count_both(gpu, cpu, st, b, b + 2000, target=target, mask=mask)
    assert ev_g == ev_c == 2000
    f_g, r_g, _ = gpu.scan_pool(5, st, target, mask, b, b + 2000, seed=SEED)
    f_c, _, _ = cpu.scan_pool(5, st, target, mask, b, b + 2000, seed=SEED)
    assert f_g == f_c
    assert f_g  # a mask inside the target's ones is realised by constants
    orc.assert_hit_valid(5, st, r_g, target, mask)
    assert b <= orc.checked_rank(orc.hit_ids(5, r_g), n) < b + 2000
    hits = check_ranks(gpu, cpu, st, ints, n, target, mask,
                       rng.sample(range(total), 40))
    assert hits == 40


# ---------------------------------------------------------------------------
# 6. The two pool sizes next to the crossover.
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["below", "above"])
def test_threshold_neighbours(engines, side):
    """Pool WIDE_MIN_ROW + 2 has no row that takes the wide walk, pool
    WIDE_MIN_ROW + 4 has one: both agree with the CPU, so the two walks
    agree where they meet."""
    n = WIDE_MIN_ROW + (2 if side == "below" else 4)
    if side == "below":
        assert n - 3 <= WIDE_MIN_ROW
    else:
        assert_wide(n)
    gpu, cpu = engines
    st, _, ints = pool(n)
    total = math.comb(n, 5)
    ev_g, ev_c = count_both(gpu, cpu, st, 0, total)
    assert ev_g == ev_c == total
    target = aes_target()
    rng = random.Random(0x7E5 + n)
    for r in rng.sample(range(total), 100):
        f_g, r_g, ev_g = gpu.scan_pool(5, st, target, FULL, r, r + 1, seed=SEED)
        f_c, r_c, _ = cpu.scan_pool(5, st, target, FULL, r, r + 1, seed=SEED)
        assert ev_g == 1 and f_g == f_c, (r, ev_g, f_g, f_c)
        if f_g:
            assert list(r_g) == list(r_c), (r, list(r_g), list(r_c))
    # The same ranks under a sparse mask, where hits are common.
    mask = orc.sparse_mask(0x7E5, 12, target)
    hits = check_ranks(gpu, cpu, st, ints, n, target, mask,
                       rng.sample(range(total), 100))
    print(side, "pool", n, "sparse-mask hits in 100 ranks:", hits)
