"""Fixtures of the large-pool scan tests (tests/test_gpu_large_pools.py),
with their CPU references: sentinel lists, planted targets, windows, and the
CPU scan of every window, computed once per (kind, pool) and never changed.
tests/test_oracle.py asserts on the CPU what the GPU tests build on.

Kinds as in _oracle_onesided.py: 3, 4, 5, 7, and "s" for the shared-input
scan. Pools are those of test_gpu_sentinels.pool (seed 0x5E17 + n), which
are full of dependent gates, so that a window around a planted combination
usually holds further hits.
"""

import functools
import itertools
import math
import random

import _oracle as orc
import _oracle_onesided as one
import _oracle_shared as osh
import test_gpu_sentinels as sen
from sboxgates_amd.ops import gen_lut_ttable

FULL = sen.FULL
SEED = sen.SEED
HALF_WINDOW = 2000
width, scan, hit_ids, kind_id = one.width, one.scan, one.hit_ids, one.kind_id
layout, engine_kind = one.layout, one.engine_kind


def case_id(case):
    return "%s-pool%d" % (kind_id(case[0]), case[1])


def cpu_engine(kind):
    return orc.cpu_engine(engine_kind(kind))


def threes(kind):
    return orc.threes_default() if kind == 4 else None


def assert_hit_valid(kind, st, res, target, mask=FULL):
    orc.assert_hit_valid(layout(kind), st, res, target, mask, threes(kind))


# --- sentinels --------------------------------------------------------------

def sept_sentinels(n):
    """test_gpu_sentinels.sept_sentinels and the two ends of the first id's
    range: the last quad, and the first combination with a = 1."""
    combs = set(sen.sept_sentinels(n))
    combs.add(tuple(range(n - 7, n)))
    combs.add(tuple(range(1, 8)))
    return sorted(combs)


def shared_sentinels(n):
    """The 4-gate analogue of test_gpu_sentinels.quint_sentinels: the first
    and the last combination, and for six triples the rows' first, a middle
    and their last d."""
    combs = {tuple(range(4)), tuple(range(n - 4, n))}
    rng = random.Random(0x4000 + n)
    triples = [(0, 1, 2), (0, 1, n - 3), (0, 1, n - 2), (n - 4, n - 3, n - 2)]
    triples += [tuple(sorted(rng.sample(range(n - 1), 3))) for _ in range(2)]
    for t in triples:
        c = t[2]
        for d in (c + 1, (c + 1 + n - 1) // 2, n - 1):
            assert c < d < n
            combs.add(t + (d,))
    return sorted(combs)


def plant_shared(tabs, rng):
    """(target, shape): LUT(fi; LUT(fo; x, y, z), d, s) over the four gates
    `tabs` (ascending ids) in a drawn shape, s drawn from the triple with
    it, neither constant."""
    full = orc.tt_int(FULL)
    for _ in range(100):
        shape = rng.randrange(12)
        triple, r, s = osh.shape_positions(shape)
        t_o = gen_lut_ttable(rng.randrange(1, 255), *(tabs[j] for j in triple))
        target = gen_lut_ttable(rng.randrange(1, 255), t_o, tabs[r], tabs[s])
        if 0 < orc.tt_int(target) & full < full:
            return target, shape
    raise AssertionError("no non-constant planted target")


def plant(kind, tabs, rng):
    if kind == "s":
        return plant_shared(tabs, rng)[0]
    return sen.plant(kind, tabs, rng, threes(kind))


def sentinels(kind, n):
    if kind in (3, 4):
        return sen.triple_sentinels(n)
    if kind == 5:
        return sen.quint_sentinels(n)
    return shared_sentinels(n) if kind == "s" else sept_sentinels(n)


# --- 4. ordered sentinels: windows of +-2000 ranks --------------------------

# (kind, pool): k=5 at 450 and 500 runs k_scan5_wave, at 120 the batch
# kernel's wide walk.
ORDERED_CASES = [(3, 500), (4, 500), (5, 450), (5, 500), (5, 120),
                 ("s", 450), ("s", 500), (7, 200), (7, 500)]


@functools.lru_cache(maxsize=None)
def ordered_windows(case):
    """Per sentinel: (combination, its rank, target, begin, end)."""
    kind, n = case
    _, tabs = sen.pool(n)
    total = math.comb(n, width(kind))
    rng = random.Random(0x0D00 + 16 * n + width(kind))
    out = []
    for comb in sentinels(kind, n):
        r = orc.checked_rank(list(comb), n)
        target = plant(kind, [tabs[i] for i in comb], rng)
        out.append((comb, r, target, max(0, r - HALF_WINDOW),
                    min(total, r + HALF_WINDOW + 1)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def ordered_reference(case):
    """Per window of ordered_windows: (CPU found, CPU res, the window holds
    a second CPU hit)."""
    kind, n = case
    st, _ = sen.pool(n)
    cpu = cpu_engine(kind)
    out = []
    for comb, r, target, begin, end in ordered_windows(case):
        f_c, r_c, _ = scan(cpu, kind, st, target, FULL, begin, end, seed=SEED)
        assert f_c, (case, comb)
        first = orc.checked_rank(hit_ids(kind, r_c), n)
        assert begin <= first <= r, (case, comb, first)
        again = scan(cpu, kind, st, target, FULL, first + 1, end, seed=SEED)
        out.append((True, tuple(r_c), bool(again[0])))
    return tuple(out)


def multi_hit_windows(case):
    """(windows with a second hit, windows)."""
    ref = ordered_reference(case)
    return sum(1 for row in ref if row[2]), len(ref)


# --- 3. windows that begin anywhere in the rank space -----------------------

ANYWHERE_CASES = [(7, 500), (5, 450), (5, 500), ("s", 500)]
DRAWS = 20


@functools.lru_cache(maxsize=None)
def anywhere_windows(case):
    """60 stratified prefixes (all ids of a combination but the last): 20
    uniform over sorted id tuples, 20 with the first id in the top tenth of
    the pool, 20 uniform over ranks. Per prefix (b, row end, window end):
    b is the first rank of the prefix's row, row end its last, and the
    window is [b, b + n) clipped to the space."""
    kind, n = case
    k = width(kind)
    total = math.comb(n, k)
    rng = random.Random(0xA000 + 16 * n + k)
    prefixes = []
    for _ in range(DRAWS):
        prefixes.append(sorted(rng.sample(range(n - 1), k - 1)))
    for _ in range(DRAWS):
        prefixes.append(sorted(rng.sample(range(n - n // 10, n - 1), k - 1)))
    for _ in range(DRAWS):
        prefixes.append(orc.unrank(rng.randrange(total), n, k)[:-1])
    out = []
    for p in prefixes:
        assert p[0] >= 0 and p[-1] <= n - 2 and p == sorted(set(p))
        b = orc.checked_rank(p + [p[-1] + 1], n)
        row_end = orc.checked_rank(p + [n - 1], n)
        assert row_end - b == n - 2 - p[-1]
        out.append((b, row_end, min(total, b + n)))
    assert sum(1 for p in prefixes if p[0] >= n - n // 10) >= DRAWS
    return tuple(out)


def anywhere_target(n):
    """The table of gate n - 1: every combination that holds the gate hits,
    so each row's last rank does."""
    return sen.pool(n)[1][n - 1]


@functools.lru_cache(maxsize=None)
def anywhere_reference(case):
    """Per window: (CPU found, CPU res, CPU evaluated, rank of the CPU hit,
    the CPU finds a further hit behind the row's end)."""
    kind, n = case
    st, _ = sen.pool(n)
    cpu = cpu_engine(kind)
    target = anywhere_target(n)
    out = []
    for b, row_end, end in anywhere_windows(case):
        f_c, r_c, ev_c = scan(cpu, kind, st, target, FULL, b, end, seed=SEED)
        assert f_c, (case, b)
        rank = orc.checked_rank(hit_ids(kind, r_c), n)
        later = row_end + 1 < end and bool(
            scan(cpu, kind, st, target, FULL, row_end + 1, end, seed=SEED)[0])
        out.append((True, tuple(r_c), ev_c, rank, later))
    return tuple(out)


# --- 5. exclusion counts ----------------------------------------------------

EXCL_POOL = 500
EXCL_WINDOW = 200_000
EXCL_KINDS = (7, "s")


def exclusion_sets():
    six = 0
    for g in random.Random(0x500).sample(range(64), 6):
        six |= 1 << g
    return [1 << 63, 1 << 0 | 1 << 63, six]


def exclusion_windows(kind):
    """Begins of the windows of EXCL_WINDOW ranks: at 0 (for k=7 inside one
    quad of C(496, 3) triples, which the host slices), across the first
    change of the first id, and at the end of the space."""
    n, k, w = EXCL_POOL, width(kind), EXCL_WINDOW
    total = math.comb(n, k)
    a_change = total - math.comb(n - 1, k)   # first rank with a = 1
    assert orc.unrank(a_change - 1, n, k)[0] == 0
    assert orc.unrank(a_change, n, k)[0] == 1
    assert w // 2 < a_change < total - 2 * w
    return [0, a_change - w // 2, total - w]


def last_window_walk(kind):
    """The exclusion-relevant ids (below 64) of every combination of the
    last window, as bit sets, from a walk in Python."""
    n, k, w = EXCL_POOL, width(kind), EXCL_WINDOW
    comb = orc.unrank(math.comb(n, k) - w, n, k)
    it = itertools.dropwhile(lambda c: list(c) != comb,
                             itertools.combinations(range(comb[0], n), k))
    last = [sum(1 << g for g in c if g < 64) for c in it]
    assert len(last) == w
    return last
