"""k_scan5_wave's per-triple set-up (gfx950): one triple per lane for a whole
chunk, list heads in registers, prefix cells and complete position lists
built on demand. Against cpu_scan5 and the independent oracle.

The wave kernel is forced for every pool. Each case is built so that one of
the set-up's paths runs, and establishes that on the CPU with the code the
kernel compiles (_core.scan5_screen_cell, sbg/scan5_cell.hpp): sparse masks
(few cared-for positions, the rest don't-care) give a named triple's screen
cell sides of a chosen size. A side of at most 16 positions is walked from
the heads alone; a longer one needs the complete lists as soon as some
candidate of a step survives 16 positions of each side, which a planted
candidate always does. Whatever passes the screen takes the rare path, which
needs the eight prefix cells: with sparse masks that is most candidates.

Every case compares, over the same window: `evaluated` of count_all scans,
the verdict of plain scans, and the ordered engine's result (the lowest
hit) with the CPU engine's; hits are validated by the oracle, which also
says that the ranks just below the hit are none.
"""

import functools
import itertools
import math
import random

import pytest

import _oracle as orc
from sboxgates_amd import _core
from test_scan5_aligned import FULL, SEED, aes_target, bits, plant, pool

pytestmark = pytest.mark.gpu

POOLS = (65, 100, 130)
ALL = (1 << 256) - 1
HEAD = 16  # positions a side that the walk has in registers


@pytest.fixture(scope="module", autouse=True)
def wave_kernel():
    old = _core.scan5_wave_min_pool()
    _core.set_scan5_wave_min_pool(_core.SCAN5_WIDE_MIN_ROW + 4)
    yield
    _core.set_scan5_wave_min_pool(old)


@pytest.fixture(scope="module")
def engines(wave_kernel):
    if not _core.gpu_available():
        pytest.skip("no GPU")
    gpu, cpu = orc.make_pair(True)
    gpu_ord = orc.rijndael_engine(True, gpu="force", ordered=True)
    assert gpu.gpu_active and gpu_ord.gpu_active
    return gpu, cpu, gpu_ord


# --- CPU side: cells, masks, windows ----------------------------------------

def cell_of(ints, triple, u):
    m = ALL
    for bit, g in zip((4, 2, 1), triple):
        m &= ints[g] if u & bit else ~ints[g] & ALL
    return m


def screen_cell(tabs, triple, target, mask):
    """(live, u0, c1, c0) as the kernel's set-up computes them."""
    t, m = orc.tt_int(target), orc.tt_int(mask)
    return tuple(_core.scan5_screen_cell(
        tabs[triple[0]], tabs[triple[1]], tabs[triple[2]],
        orc.tt_bytes(t & m), orc.tt_bytes(~t & m & ALL)))


def span(n, triple):
    c = triple[2]
    return (orc.checked_rank(triple + (c + 1, c + 2), n),
            orc.checked_rank(triple + (n - 2, n - 1), n) + 1)


@functools.lru_cache(maxsize=None)
def roomy_triple(n, target, side):
    """The first triple (with a long row) that has a prefix cell with at
    least `side` target-1 and `side` target-0 positions: (triple, cell)."""
    ints = pool(n)[2]
    t = orc.tt_int(target)
    for triple in itertools.combinations(range(n - 45), 3):
        for u in range(8):
            m = cell_of(ints, triple, u)
            if (bin(m & t).count("1") >= side and
                    bin(m & ~t).count("1") >= side):
                return triple, u
    raise AssertionError("no roomy cell")


def cell_mask(n, target, triple, u, k1, k0, rng, words=None):
    """A mask that cares for k1 target-1 and k0 target-0 positions of the
    triple's cell u and for nothing else, so that u is the only live cell
    and the screen cell, with sides of exactly k1 and k0. words: table
    words (64 positions each) the positions must lie in."""
    st, tabs, ints = pool(n)
    t = orc.tt_int(target)
    m = cell_of(ints, triple, u)
    if words is not None:
        m &= sum(((1 << 64) - 1) << (64 * w) for w in words)
    p1, p0 = orc.positions(m & t), orc.positions(m & ~t)
    assert len(p1) >= k1 and len(p0) >= k0, (len(p1), len(p0))
    mask = sum(1 << p for p in rng.sample(p1, k1) + rng.sample(p0, k0))
    mask = orc.tt_bytes(mask)
    assert screen_cell(tabs, triple, target, mask) == (1 << u, u, k1, k0)
    return mask


def screen_survivors(n, triple, target, mask, heads_only=False, d_min=None):
    """Pairs (d, e) of the triple that pass the screen cell's test: they take
    the rare path. heads_only: pairs without a conflict among the first
    HEAD positions of each side, which is where the walk leaves the heads;
    if a side is longer, such a pair makes the walk read the complete
    lists. d_min: rows from d_min on only."""
    _, tabs, ints = pool(n)
    _, u0, _, _ = screen_cell(tabs, triple, target, mask)
    t, m = orc.tt_int(target), orc.tt_int(mask)
    cell = cell_of(ints, triple, u0)
    h1, h0 = cell & t & m, cell & ~t & m
    if heads_only:
        h1 = sum(1 << p for p in orc.positions(h1)[:HEAD])
        h0 = sum(1 << p for p in orc.positions(h0)[:HEAD])
    out = []
    for d in range(max(triple[2] + 1, d_min or 0), n - 1):
        for e in range(d + 1, n):
            ok = True
            for xd in (ints[d], ~ints[d]):
                for xe in (ints[e], ~ints[e]):
                    if h1 & xd & xe and h0 & xd & xe:
                        ok = False
            if ok:
                out.append((d, e))
    return out


def past_heads(n, triple, target, mask, d_min=None):
    """True if the triple's walk must read the complete lists: a side of
    its screen cell is longer than the heads and some pair survives them."""
    _, _, c1, c0 = screen_cell(pool(n)[1], triple, target, mask)
    return (min(c1, c0) > 0 and max(c1, c0) > HEAD and
            len(screen_survivors(n, triple, target, mask, True, d_min)) > 0)


def compare(engines, n, target, mask, b, e, excl=0, expect_found=None):
    """One window, all three scans, GPU against CPU and oracle. Returns the
    hit's rank, or None."""
    gpu, cpu, gpu_ord = engines
    st, _, ints = pool(n)
    kw = dict(seed=SEED, excl=excl)
    _, _, ev_g = gpu.scan_pool(5, st, target, mask, b, e, count_all=True, **kw)
    _, _, ev_c = cpu.scan_pool(5, st, target, mask, b, e, count_all=True, **kw)
    assert ev_g == ev_c, (n, b, e, ev_g, ev_c)
    if excl == 0:
        assert ev_g == e - b
    f_c, r_c, _ = cpu.scan_pool(5, st, target, mask, b, e, **kw)
    f_g, r_g, _ = gpu.scan_pool(5, st, target, mask, b, e, **kw)
    f_o, r_o, _ = gpu_ord.scan_pool(5, st, target, mask, b, e, **kw)
    assert bool(f_g) == bool(f_c) == bool(f_o), (n, b, e, f_g, f_o, f_c)
    if expect_found is not None:
        assert bool(f_c) == expect_found, (n, b, e)
    if not f_c:
        return None
    orc.assert_hit_valid(5, st, r_g, target, mask)
    orc.assert_hit_valid(5, st, r_o, target, mask)
    assert list(r_o) == list(r_c), (n, b, e, list(r_o), list(r_c))
    ids = orc.hit_ids(5, r_o)
    r = orc.checked_rank(ids, n)
    assert b <= r < e
    t, m = orc.tt_int(target), orc.tt_int(mask)
    assert orc.found5([ints[i] for i in ids], t, m)
    for below in range(max(b, r - 24), r):  # the lowest: none just below it
        comb = orc.checked_unrank(below, n, 5)
        if excl and any(i < 64 and (excl >> i) & 1 for i in comb):
            continue
        assert not orc.found5([ints[i] for i in comb], t, m), (n, comb)
    return r


# --- 1. Heads exactly at the boundary ---------------------------------------

@pytest.mark.parametrize("side", [1, 2, 3, 4, 15, 16, 17, 33])
@pytest.mark.parametrize("n", POOLS)
def test_head_boundary(engines, n, side):
    """The named triple's screen cell gets sides of exactly `side` and
    side + 1 positions, both ways round, its only live cell (cell_mask
    asserts it through _core.scan5_screen_cell). The target is
    f(a, b, c) ^ e (roomy_many_hits), so the pairs (d, e) contradict nowhere
    and survive any number of positions: asserted on the CPU as pairs that
    pass the first 16 positions of each side. With a side of 16 or fewer
    the walk then ends inside the heads; with 17 (one real position and
    three pad bytes behind the heads) and with 33 and 34 (a target-0 list
    that starts past byte 32) it reads the complete lists, built on demand
    (past_heads asserts which of the two it is). The window is the triple
    and its successor, so the next triple starts from the first one's
    leftovers."""
    triple, u, target, _ = roomy_many_hits(n, 34)
    rng = random.Random(100 * n + side)
    b, e = span(n, triple)
    e = span(n, tuple(orc.checked_unrank(orc.checked_rank(triple, n) + 1, n, 3)))[1]
    for k1, k0 in ((side, side + 1), (side + 1, side)):
        mask = cell_mask(n, target, triple, u, k1, k0, rng)
        assert len(screen_survivors(n, triple, target, mask, True)) > 0
        assert past_heads(n, triple, target, mask) == (side + 1 > HEAD)
        compare(engines, n, target, mask, b, e, expect_found=True)


# --- 2. Positions in single table words -------------------------------------

@pytest.mark.parametrize("words", [(3,), (0,), (0, 3)])
@pytest.mark.parametrize("n", POOLS)
def test_positions_in_few_table_words(engines, n, words):
    """Every cared-for position lies in the named 64-position words of the
    table (word 3: positions 192..255, the last dwords a lane looks at when
    it collects a head). All positions of those words are cared for, so
    several cells are live and the screen cell has sides of a few
    positions; established by scan5_screen_cell over the window's triples."""
    target = aes_target()
    st, tabs, _ = pool(n)
    mask = orc.tt_bytes(sum(((1 << 64) - 1) << (64 * w) for w in words))
    t0 = math.comb(n, 3) // 3
    triples = [tuple(orc.checked_unrank(t, n, 3)) for t in range(t0, t0 + 3)]
    assert all(t[2] <= n - 3 for t in triples)
    for triple in triples:
        live, _, c1, c0 = screen_cell(tabs, triple, target, mask)
        assert live != 0 and 0 < min(c1, c0) <= 32 * len(words)
    compare(engines, n, target, mask, span(n, triples[0])[0],
            span(n, triples[-1])[1])
    # One cell only, all its positions inside these words.
    triple, u = roomy_triple(n, target, 34)
    m = cell_of(pool(n)[2], triple, u)
    m &= orc.tt_int(mask)
    p1 = bin(m & orc.tt_int(target)).count("1")
    p0 = bin(m & ~orc.tt_int(target)).count("1")
    assert min(p1, p0) >= 1
    mask1 = cell_mask(n, target, triple, u, p1, p0, random.Random(n),
                      words=words)
    compare(engines, n, target, mask1, *span(n, triple))


# --- 3. Triples without a live cell next to triples with one ----------------

@pytest.mark.parametrize("n", POOLS)
def test_chunk_with_and_without_live_cells(engines, n):
    """A mask of three positions (two target-1, one target-0): a triple has
    a live cell only if the target-0 position shares a cell with a target-1
    one. The window is a run of 16 consecutive triples, two chunks of a
    small scan, chosen so that its first eight hold both kinds
    (scan5_screen_cell says live == 0, screen cell 7, for the ones without).
    Without a live cell everything passes the screen and takes the rare
    path."""
    target = aes_target()
    st, tabs, _ = pool(n)
    t = orc.tt_int(target)
    rng = random.Random(n)
    mask = orc.tt_bytes(sum(1 << p for p in
                            rng.sample(orc.positions(t), 2) +
                            rng.sample(orc.positions(~t & ALL), 1)))
    units = math.comb(n, 3)
    for t0 in range(units // 4, units // 4 + 4000):
        run = [tuple(orc.checked_unrank(x, n, 3)) for x in range(t0, t0 + 16)]
        if any(x[2] > n - 3 for x in run):
            continue
        kinds = [screen_cell(tabs, x, target, mask) for x in run[:8]]
        dead = [k for k in kinds if k[0] == 0]
        if dead and len(dead) < 8:
            assert all(k[1] == 7 for k in dead)
            break
    else:
        raise AssertionError("no mixed chunk")
    compare(engines, n, target, mask, span(n, run[0])[0], span(n, run[-1])[1])


# --- 4. Dead triples between live ones --------------------------------------

@pytest.mark.parametrize("n", POOLS)
def test_chunk_with_dead_triples(engines, n):
    """Triples (0, 1, c) for consecutive c, with c = 6 and c = 9 excluded:
    their lanes set nothing up and the walk skips them, between live
    triples. Once with a sparse mask (the cell of (0, 1, 5) with sides of 10
    and 11 positions, cell_mask: the live triples run from the heads) and
    once with the full mask."""
    target = aes_target()
    st, tabs, ints = pool(n)
    excl = bits([6, 9])
    rng = random.Random(3 * n)
    # One mask for the run: the cell of (0, 1, 5) with 10 + 11 positions.
    u = max(range(8), key=lambda u: min(
        bin(cell_of(ints, (0, 1, 5), u) & orc.tt_int(target)).count("1"),
        bin(cell_of(ints, (0, 1, 5), u) & ~orc.tt_int(target)).count("1")))
    mask = cell_mask(n, target, (0, 1, 5), u, 10, 11, rng)
    b = span(n, (0, 1, 4))[0]
    e = span(n, (0, 1, 11))[1]
    compare(engines, n, target, mask, b, e, excl=excl)
    compare(engines, n, aes_target(), FULL, b, e, excl=excl,
            expect_found=False)


# --- 5. Survivors -----------------------------------------------------------

def middle_triple(n):
    """A triple in mid-pool whose rows are long."""
    return (n // 5, n // 4, n // 3)


@functools.lru_cache(maxsize=None)
def roomy_many_hits(n, side):
    """(triple, cell, target, e): the target is f(a, b, c) ^ e for a gate
    e behind the triple, so every pair (d, e) with c < d < e hits, and the
    triple's cell has at least `side` target-1 and `side` target-0
    positions."""
    ints = pool(n)[2]
    full = orc.tt_int(FULL)
    for triple in itertools.combinations(range(n - 45), 3):
        f = ints[triple[0]] & ints[triple[1]] | ints[triple[2]]
        for e in range(n - 2, triple[2] + 20, -1):
            t = (f ^ ints[e]) & full
            if not 0 < t < full:
                continue
            for u in range(8):
                m = cell_of(ints, triple, u)
                if (bin(m & t).count("1") >= side and
                        bin(m & ~t).count("1") >= side):
                    return triple, u, orc.tt_bytes(t), e
    raise AssertionError("no roomy cell")


@pytest.mark.parametrize("n", POOLS)
def test_one_survivor(engines, n):
    """Full mask, a target planted on one combination: its triple builds the
    prefix cells for the one candidate that passes the screen (the CPU
    finds the same lowest hit)."""
    _, tabs, _ = pool(n)
    rng = random.Random(5 * n)
    triple = middle_triple(n)
    c = triple[2]
    d = rng.randrange(c + 1, n - 1)
    comb = triple + (d, rng.randrange(d + 1, n))
    target = plant(tabs, comb, rng)
    b, e = span(n, triple)
    r = compare(engines, n, target, FULL, b, e, expect_found=True)
    assert r <= orc.checked_rank(comb, n)


@pytest.mark.parametrize("n", POOLS)
def test_survivors_in_different_lanes_of_one_step(engines, n):
    """The target is LUT(LUT(a, b, c), e): a function of the triple and one
    more gate e, so the pairs (d, e) hit for every row d < e. Rows are
    lanes, and the rows just below e share e's word group and a step: many
    lanes of that step survive at once."""
    _, tabs, ints = pool(n)
    rng = random.Random(7 * n)
    triple = middle_triple(n)
    e_gate = n - 2
    full = orc.tt_int(FULL)
    f = ints[triple[0]] & ints[triple[1]] | ints[triple[2]]
    value = (f ^ ints[e_gate]) & full
    assert 0 < value < full
    target = orc.tt_bytes(value)
    b, e = span(n, triple)
    r = compare(engines, n, target, FULL, b, e, expect_found=True)
    assert r <= orc.checked_rank(triple + (triple[2] + 1, e_gate), n)


@functools.lru_cache(maxsize=None)
def consecutive_case(n):
    """(first, second, target, mask) for test_survivors_in_consecutive_triples.
    first = (a, b, c), second = (a, b, c + 1), x the gate c + 1, e the gate
    n - 2, target = ((a & b) | x) ^ e. The mask cares for 18 + 18 positions
    of one cell of `first` on which a & b is 0 and x is constant: there the
    target is e or ~e, the cell is the screen cell of both triples, and every
    pair (d, e) survives it. It also cares for up to 8 positions of every
    kind (x, e) in the other cells of `first` on which a & b is 0: there x
    varies, so to `first` the target is no function of its cells, while to
    `second` it is; their sides stay below 18, so the screen cell stays.
    The first such case in which the CPU engine finds no hit in `first`
    behind its first row."""
    st, _, ints = pool(n)
    cpu = orc.cpu_engine(5)
    te = ints[n - 2]
    rng = random.Random(11 * n)

    def pc(v):
        return bin(v).count("1")

    for a, b in itertools.combinations(range(n - 50), 2):
        for c in range(b + 1, n - 48):
            x = ints[c + 1]
            t = ((ints[a] & ints[b] | x) ^ te) & ALL
            for u, xv in itertools.product(range(8), (x, ~x & ALL)):
                if u & 4 and u & 2:
                    continue
                m1 = cell_of(ints, (a, b, c), u) & xv
                if pc(m1 & t) < 18 or pc(m1 & ~t) < 18:
                    continue
                p1, p0 = orc.positions(m1 & t), orc.positions(m1 & ~t)
                pos = rng.sample(p1, 18) + rng.sample(p0, 18)
                for u2 in range(8):
                    if u2 == u or (u2 & 4 and u2 & 2):
                        continue
                    m2 = cell_of(ints, (a, b, c), u2)
                    for xx in (x, ~x & ALL):
                        for tt in (te, ~te & ALL):
                            part = orc.positions(m2 & xx & tt)
                            pos += rng.sample(part, min(8, len(part)))
                mask = orc.tt_bytes(sum(1 << p for p in pos))
                target = orc.tt_bytes(t)
                # No hit in `first` behind its first row.
                begin = orc.checked_rank((a, b, c, c + 2, c + 3), n)
                mid = span(n, (a, b, c + 1))[0]
                if not cpu.scan_pool(5, st, target, mask, begin, mid,
                                     seed=SEED)[0]:
                    return (a, b, c), (a, b, c + 1), target, mask
    raise AssertionError("no case")


@pytest.mark.parametrize("n", POOLS)
def test_survivors_in_consecutive_triples(engines, n):
    """Two consecutive triples whose screen cells both have sides of 18
    positions (consecutive_case; scan5_screen_cell says so), in a window
    that begins behind the first triple's first row. In both, pairs survive
    the heads (past_heads), so both build the complete lists, and the pairs
    that survive the whole screen build the prefix cells. The first triple
    has no hit from that row on (the CPU engine says so) and the second has
    many, so the window's lowest hit is a verdict of the second triple,
    reached after the wave has built the first one's lists and cells: it
    must come from the second triple's own."""
    gpu, cpu, _ = engines
    st, tabs, _ = pool(n)
    first, second, target, mask = consecutive_case(n)
    c = first[2]
    for triple in (first, second):
        _, _, c1, c0 = screen_cell(tabs, triple, target, mask)
        assert min(c1, c0) > HEAD, (triple, c1, c0)
    assert past_heads(n, first, target, mask, d_min=c + 2)
    assert past_heads(n, second, target, mask)
    assert len(screen_survivors(n, first, target, mask, d_min=c + 2)) > 0
    begin = orc.checked_rank(first + (c + 2, c + 3), n)
    mid, end = span(n, second)
    f_c, _, _ = cpu.scan_pool(5, st, target, mask, begin, mid, seed=SEED)
    assert not f_c
    r = compare(engines, n, target, mask, begin, end, expect_found=True)
    assert r >= mid
    compare(engines, n, target, mask, begin, mid, expect_found=False)


@pytest.mark.parametrize("n", POOLS)
def test_survivor_behind_long_lists(engines, n):
    """A planted target, and a mask that gives the planted triple's screen
    cell sides of 20 and 24 positions (cell_mask), its only live cell. The
    planted candidate contradicts nowhere, so its step walks all 24
    positions: past the heads, the lists are built; then it takes the rare
    path, the cells are built, in the same triple."""
    _, tabs, ints = pool(n)
    rng = random.Random(13 * n)
    triple, u = roomy_triple(n, aes_target(), 34)
    c = triple[2]
    for _ in range(200):
        d = rng.randrange(c + 1, n - 1)
        comb = triple + (d, rng.randrange(d + 1, n))
        target = plant(tabs, comb, rng)
        t = orc.tt_int(target)
        us = [v for v in range(8)
              if bin(cell_of(ints, triple, v) & t).count("1") >= 24 and
              bin(cell_of(ints, triple, v) & ~t).count("1") >= 24]
        if us:
            break
    else:
        raise AssertionError("no planted target with a roomy cell")
    mask = cell_mask(n, target, triple, us[0], 20, 24, rng)
    assert comb[3:] in screen_survivors(n, triple, target, mask)
    b, e = span(n, triple)
    r = compare(engines, n, target, mask, b, e, expect_found=True)
    assert r <= orc.checked_rank(comb, n)


# --- 6. Ordered scans with hits in two chunks --------------------------------

@pytest.mark.parametrize("n", POOLS)
def test_ordered_hits_in_two_chunks(engines, n):
    """The target is a function of three gates g < d < e, so every
    combination that holds them hits: in the triples (0, 1, g) and
    (g, g + 1, g + 2), hundreds of chunks apart. The lowest rank inside the
    window wins, from both starts."""
    _, cpu, gpu_ord = engines
    st, _, ints = pool(n)
    total = math.comb(n, 5)
    g, d, e = 3, n - 7, n - 2
    full = orc.tt_int(FULL)
    value = (ints[g] & ints[d]) ^ ints[e]
    assert 0 < value & full < full
    target = orc.tt_bytes(value)
    hit_lo = orc.checked_rank((0, 1, g, d, e), n)
    hit_hi = orc.checked_rank((g, g + 1, g + 2, d, e), n)
    assert (orc.checked_rank((g, g + 1, g + 2), n) -
            orc.checked_rank((0, 1, g), n)) >= 64
    for begin in (0, hit_lo + 1, hit_hi - 1000):
        f_g, r_g, _ = gpu_ord.scan_pool(5, st, target, FULL, begin, total,
                                        seed=SEED)
        f_c, r_c, _ = cpu.scan_pool(5, st, target, FULL, begin,
                                    min(total, begin + 500_000), seed=SEED)
        assert f_g and f_c, (n, begin)
        assert list(r_g) == list(r_c), (n, begin, list(r_g), list(r_c))
        orc.assert_hit_valid(5, st, r_g, target, FULL)


# --- 7. Windows inside a triple with on-demand lists -------------------------

@pytest.mark.parametrize("n", POOLS)
def test_windows_inside_a_triple(engines, n):
    """Windows that begin and end inside one triple. Its screen cell has
    sides of 18 and 19 positions (cell_mask), and the target makes every
    pair (d, e) hit for one gate e (roomy_many_hits; screen_survivors
    counts them), so each step that holds one walks past the heads: the
    lists are built on demand in whichever step of the window comes
    first."""
    triple, u, target, e_gate = roomy_many_hits(n, 19)
    rng = random.Random(17 * n)
    mask = cell_mask(n, target, triple, u, 18, 19, rng)
    m = n - 1 - triple[2]
    assert len(screen_survivors(n, triple, target, mask)) >= e_gate - triple[2] - 1
    assert past_heads(n, triple, target, mask)
    b, e = span(n, triple)
    for lo, hi in ((1, e - b - 1), (m - 2, m + 70), (m + 63, m + 64),
                   ((e - b) // 2, (e - b) // 2 + 129), (e - b - 3, e - b)):
        compare(engines, n, target, mask, b + lo, b + hi)
