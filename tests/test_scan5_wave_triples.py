"""k_scan5 wide kernels (gfx950), above all the one whose waves take triples
off the queue in chunks (k_scan5_wave): against cpu_scan5 and the
independent oracle. Every test runs twice: with the wave-owned kernel on
every pool that has a long row, and with the kernels the host chooses by
itself (the batch kernel below _core.SCAN5_WAVE_MIN_POOL gates).

A wave takes up to CHUNK = 64 consecutive triples at a time, counted from the
first triple of the scan's range; small scans take smaller chunks. These
tests pin what a caller sees (verdicts, results, evaluated counts) around
the triples whose index is a multiple of CHUNK or of the chunk size the pool's
full scan uses, plus and minus one: windows that begin and end there, planted
targets whose realising triple is the first or the last of a chunk, a
short-row triple (rows of 40 or fewer) among wide ones and the reverse, the
pool's last triple, exclusion sets that kill triples in mid-chunk, and ordered
scans with hits in several chunks. They hold for any layout of the queue.

Pools: 65 (rows above and below 41 inside one chunk), 100, 130 (several row
blocks and word groups per triple); 300 for chunks of 64 in a full scan.
"""

import functools
import math
import random

import pytest

import _oracle as orc
from sboxgates_amd import _core
from test_scan5_aligned import FULL, SEED, aes_target, bits, plant, pool

pytestmark = pytest.mark.gpu

CHUNK = 64
WIDE_MIN_ROW = _core.SCAN5_WIDE_MIN_ROW
POOLS = (65, 100, 130)
BIG = 300  # C(300, 3) triples: its full scan takes chunks of 64


@pytest.fixture(scope="module", autouse=True, params=["wave", "default"])
def kernel_choice(request):
    old = _core.scan5_wave_min_pool()
    assert old == _core.SCAN5_WAVE_MIN_POOL
    if request.param == "wave":
        _core.set_scan5_wave_min_pool(WIDE_MIN_ROW + 4)
    yield request.param
    _core.set_scan5_wave_min_pool(old)


@pytest.fixture(scope="module")
def engines(kernel_choice):
    if not _core.gpu_available():
        pytest.skip("no GPU")
    gpu, cpu = orc.make_pair(True)
    gpu_ord = orc.rijndael_engine(True, gpu="force", ordered=True)
    assert gpu.gpu_active and gpu_ord.gpu_active
    return gpu, cpu, gpu_ord


def triple_at(n, t):
    return tuple(orc.checked_unrank(t, n, 3))


def span(n, triple):
    """Ranks [first, last] of the triple's combinations; None if it has
    none."""
    a, b, c = triple
    if c > n - 3:
        return None
    return (orc.checked_rank((a, b, c, c + 1, c + 2), n),
            orc.checked_rank((a, b, c, n - 2, n - 1), n))


def chunk_sizes(n):
    """CHUNK and the chunk size of the pool's full scan on the largest
    grid."""
    return sorted({CHUNK, _core.scan5_chunks(math.comb(n, 3), 4 * 2048)[0][1]})


@functools.lru_cache(maxsize=None)
def boundary_triples(n):
    """Indices of triples with combinations at T - 1, T, T + 1 for a few
    multiples T of each chunk size, at the queue's start, middle and end."""
    units = math.comb(n, 3)
    out = set()
    for size in chunk_sizes(n):
        last = (units - 1) // size * size
        for T in (size, 2 * size, units // 2 // size * size, last - size, last):
            for t in (T - 1, T, T + 1):
                if 0 <= t < units and span(n, triple_at(n, t)) is not None:
                    out.add(t)
    return tuple(sorted(out))


def first_rank_at_or_after(n, t):
    units = math.comb(n, 3)
    while t < units:
        s = span(n, triple_at(n, t))
        if s is not None:
            return s[0]
        t += 1
    return math.comb(n, 5)


def count_and_verdict(gpu, cpu, st, b, e, excl=0):
    """evaluated of count_all scans and the verdict of plain ones, AES
    target, both engines alike."""
    target = aes_target()
    _, _, ev_g = gpu.scan_pool(5, st, target, FULL, b, e, seed=SEED,
                               count_all=True, excl=excl)
    _, _, ev_c = cpu.scan_pool(5, st, target, FULL, b, e, seed=SEED,
                               count_all=True, excl=excl)
    assert ev_g == ev_c, (b, e, excl, ev_g, ev_c)
    f_g, _, _ = gpu.scan_pool(5, st, target, FULL, b, e, seed=SEED, excl=excl)
    f_c, _, _ = cpu.scan_pool(5, st, target, FULL, b, e, seed=SEED, excl=excl)
    assert bool(f_g) == bool(f_c), (b, e, excl, f_g, f_c)
    return ev_g


# ---------------------------------------------------------------------------
# 1. Full range.
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", POOLS + (BIG,))
def test_full_range_count(engines, n):
    gpu = engines[0]
    st, _, _ = pool(n)
    total = math.comb(n, 5)
    found, _, ev = gpu.scan_pool(5, st, aes_target(), FULL, 0, total,
                                 seed=SEED, count_all=True)
    assert ev == total, (n, ev, total)
    assert not found


# ---------------------------------------------------------------------------
# 2. Windows on chunk boundaries.
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", POOLS)
def test_windows(engines, n):
    gpu, cpu, _ = engines
    st, _, _ = pool(n)
    total = math.comb(n, 5)
    reach = 70  # triples: more than one chunk
    windows = set()
    for t in boundary_triples(n):
        first, last = span(n, triple_at(n, t))
        far = first_rank_at_or_after(n, t + reach)
        near = first_rank_at_or_after(n, max(0, t - reach))
        for b in (first, first + 1):
            if b < far:
                windows.add((b, far))
        for e in (last, last + 1):
            if near < e:
                windows.add((near, e))
        windows.add((first, last + 1))      # exactly one triple
        if first + 1 < last:
            windows.add((first + 1, last))  # inside a single triple
    for size in chunk_sizes(n):            # exactly one chunk
        windows.add((first_rank_at_or_after(n, size),
                     first_rank_at_or_after(n, 2 * size)))
    for b, e in sorted(windows):
        assert 0 <= b < e <= total, (b, e)
        assert count_and_verdict(gpu, cpu, st, b, e) == e - b, (n, b, e)


# ---------------------------------------------------------------------------
# 3. Planted targets.
# ---------------------------------------------------------------------------
def is_short(n, triple):
    return n - 1 - triple[2] <= WIDE_MIN_ROW


def mixed_chunk(n, want_short):
    """A short-row triple (or, if not want_short, a wide one) from the first
    CHUNK-aligned run of triples that has triples of the other kind both
    before and after it."""
    units = math.comb(n, 3)
    for T in range(0, units - CHUNK, CHUNK):
        ts = [triple_at(n, t) for t in range(T, T + CHUNK)]
        kinds = [is_short(n, t) == want_short for t in ts]
        for i, t in enumerate(ts):
            if (kinds[i] and span(n, t) is not None and
                    not all(kinds[:i]) and not all(kinds[i + 1:])):
                return t
    raise AssertionError("no mixed chunk")


def chunk_edge(n, offset):
    """The triple at `offset` in a CHUNK-aligned run a third into the queue,
    or in the next run where that one has no pairs."""
    t = math.comb(n, 3) // 3 // CHUNK * CHUNK + offset
    while span(n, triple_at(n, t)) is None:
        t += CHUNK
    return triple_at(n, t)


@functools.lru_cache(maxsize=None)
def planted_triples(n):
    out = {
        "chunk_first": chunk_edge(n, 0),
        "chunk_last": chunk_edge(n, CHUNK - 1),
        "short_among_wide": mixed_chunk(n, True),
        "wide_among_short": mixed_chunk(n, False),
        "pool_last": (n - 5, n - 4, n - 3),
    }
    assert is_short(n, out["short_among_wide"])
    assert not is_short(n, out["wide_among_short"])
    return out


def aligned_begin(n, t):
    """First rank of a triple a whole number of chunks (two at least) below
    triple t; 0 where there is none."""
    for tt in range(t - 2 * CHUNK, -1, -CHUNK):
        s = span(n, triple_at(n, tt))
        if s is not None:
            return s[0]
    return 0


def comb_in(n, triple, rng):
    c = triple[2]
    d = rng.randrange(c + 1, n - 1)
    e = rng.randrange(d + 1, n)
    return triple + (d, e)


@pytest.mark.parametrize("which", ["chunk_first", "chunk_last",
                                   "short_among_wide", "wide_among_short",
                                   "pool_last"])
@pytest.mark.parametrize("n", POOLS)
def test_planted(engines, n, which):
    gpu, cpu, gpu_ord = engines
    st, tabs, _ = pool(n)
    total = math.comb(n, 5)
    rng = random.Random(1000 * n + len(which))
    triple = planted_triples(n)[which]
    comb = comb_in(n, triple, rng)
    r = orc.checked_rank(comb, n)
    target = plant(tabs, comb, rng)

    # Unordered, full range: some hit, which the oracle confirms.
    found, res, ev = gpu.scan_pool(5, st, target, FULL, 0, total, seed=SEED)
    assert found, (n, which, comb)
    assert 1 <= ev <= total
    orc.assert_hit_valid(5, st, res, target, FULL)

    # Ordered: the lowest hit, as the CPU's. The window begins a whole
    # number of chunks before the planted triple, so the triple keeps its
    # place in its chunk, and short enough for the CPU.
    t = orc.checked_rank(triple, n)
    begin = aligned_begin(n, t)
    assert begin <= r
    f_g, r_g, _ = gpu_ord.scan_pool(5, st, target, FULL, begin, total, seed=SEED)
    f_c, r_c, _ = cpu.scan_pool(5, st, target, FULL, begin, r + 1, seed=SEED)
    assert f_g and f_c, (n, which, comb)
    assert list(r_g) == list(r_c), (n, which, comb, list(r_g), list(r_c))
    orc.assert_hit_valid(5, st, r_g, target, FULL)


def test_planted_big_chunks(engines):
    """Pool 300, whose full scan takes chunks of 64: targets planted on the
    first and the last triple of a chunk."""
    gpu, cpu, gpu_ord = engines
    n = BIG
    assert _core.scan5_chunks(math.comb(n, 3), 4 * 2048)[0][1] == CHUNK
    st, tabs, _ = pool(n)
    total = math.comb(n, 5)
    rng = random.Random(n)
    for t in (50 * CHUNK, 50 * CHUNK + CHUNK - 1):
        triple = triple_at(n, t)
        comb = comb_in(n, triple, rng)
        r = orc.checked_rank(comb, n)
        target = plant(tabs, comb, rng)
        found, res, _ = gpu.scan_pool(5, st, target, FULL, 0, total, seed=SEED)
        assert found, comb
        orc.assert_hit_valid(5, st, res, target, FULL)
        # Ordered from the range's start, so chunks are those of the full
        # scan; the CPU gets the window's end: nothing hits below it unless
        # the ordered scan found it.
        f_g, r_g, _ = gpu_ord.scan_pool(5, st, target, FULL, 0, total, seed=SEED)
        assert f_g, comb
        orc.assert_hit_valid(5, st, r_g, target, FULL)
        r_found = orc.checked_rank(orc.hit_ids(5, r_g), n)
        assert r_found <= r, (comb, list(r_g))
        f_c, r_c, _ = cpu.scan_pool(5, st, target, FULL, r_found, r_found + 1,
                                    seed=SEED)
        assert f_c and list(r_c) == list(r_g), (comb, list(r_g), list(r_c))
        span_c = 1 << 20  # the CPU confirms: no hit in the ranks just below
        f_c, _, _ = cpu.scan_pool(5, st, target, FULL,
                                  max(0, r_found - span_c), r_found, seed=SEED)
        assert not f_c, comb


# ---------------------------------------------------------------------------
# 4. Exclusion sets.
# ---------------------------------------------------------------------------
EXCL = {
    "prefix_gate": [5],   # triples (., ., 5), (., 5, .): dead in mid-chunk;
                          # (5, ., .): whole chunks dead
    "a_d": [40],
    "some_e": [62, 63],
}


@pytest.mark.parametrize("which", sorted(EXCL))
@pytest.mark.parametrize("n", POOLS)
def test_exclusion(engines, n, which):
    gpu, cpu, _ = engines
    st, _, _ = pool(n)
    ids = EXCL[which]
    excl = bits(ids)
    total = math.comb(n, 5)
    _, _, ev = gpu.scan_pool(5, st, aes_target(), FULL, 0, total, seed=SEED,
                             count_all=True, excl=excl)
    assert ev == math.comb(n - len(ids), 5), (n, which, ev)
    # Against the CPU: windows of about two chunks that begin at a chunk's
    # first triple, around triples that hold an excluded gate.
    g = ids[0]
    for triple in ((0, 1, g), (0, g, g + 1), (g, g + 1, g + 2), (0, 1, 2),
                   (1, 2, 3)):
        t = orc.checked_rank(triple, n) // CHUNK * CHUNK
        b = first_rank_at_or_after(n, t)
        e = first_rank_at_or_after(n, t + 2 * CHUNK)
        ev = count_and_verdict(gpu, cpu, st, b, e, excl=excl)
        assert ev <= e - b


# ---------------------------------------------------------------------------
# 5. Ordered scans with hits in several chunks.
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(5))
@pytest.mark.parametrize("n", POOLS)
def test_ordered_lowest_of_hits_in_different_chunks(engines, n, seed):
    """The target is a function of three gates g < d < e, so every
    combination that holds them realises it: with g low there are hits in
    the triples (., ., g), (., g, .) and (g, ., .), many chunks apart. The
    lowest hit inside the window wins, as on the CPU."""
    _, cpu, gpu_ord = engines
    st, _, ints = pool(n)
    total = math.comb(n, 5)
    rng = random.Random(77 * n + seed)
    g = rng.randrange(1, 4)
    d = rng.randrange(n // 2, n - 1)
    e = rng.randrange(d + 1, n)
    full = orc.tt_int(FULL)
    value = (ints[g] & ints[d]) ^ ints[e]
    assert 0 < value & full < full
    target = orc.tt_bytes(value)
    lowest = tuple(sorted([i for i in range(4) if i != g][:2] + [g])) + (d, e)
    later = (g, g + 1, g + 2, d, e)
    hit_lo = orc.checked_rank(lowest, n)
    hit_hi = orc.checked_rank(later, n)
    assert (orc.checked_rank(later[:3], n) -
            orc.checked_rank(lowest[:3], n)) >= CHUNK  # different chunks
    cpu_reach = 500_000  # the next hit is nearer than that in every window
    for begin in (0, hit_lo + 1, hit_hi - rng.randrange(0, 200_000),
                  hit_hi + 1):
        f_g, r_g, _ = gpu_ord.scan_pool(5, st, target, FULL, begin, total,
                                        seed=SEED)
        f_c, r_c, _ = cpu.scan_pool(5, st, target, FULL, begin,
                                    min(total, begin + cpu_reach), seed=SEED)
        assert f_g and f_c, (n, seed, begin)
        assert list(r_g) == list(r_c), (n, seed, begin, list(r_g), list(r_c))
        orc.assert_hit_valid(5, st, r_g, target, FULL)
        if begin == 0:
            assert orc.checked_rank(orc.hit_ids(5, r_g), n) <= hit_lo
