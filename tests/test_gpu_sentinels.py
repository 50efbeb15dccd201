"""Sentinel tests of the GPU rank decoders and window clipping at the pool
sizes that matter: k=3 and k=4 at MAX_GATES = 500, k=5 at the benchmark's
pool 450, at 500 and at 90, k=7 at 40, 64 and 100, and k=7 exclusion
counts at pool 70, where gate ids of 64 and above exist.

Each sentinel plants a target that one chosen combination realises, under
the full mask. Its rank comes from the pure-Python unranker's inverse,
cross-checked with combination_rank. The window [r, r+1) must be a hit on
both engines and the GPU must name exactly that combination; a window of
+-2000 ranks around it (which makes the k=7 host code slice quads) must be a
valid hit on both engines, not necessarily the sentinel.
"""

import functools
import itertools
import math
import random

import pytest

import _oracle as orc
from sboxgates_amd import _core
from sboxgates_amd.ops import gen_lut_ttable, mask_for_inputs

gpu_test = pytest.mark.gpu

FULL = mask_for_inputs(8)
SEED = 5


@pytest.fixture(scope="module")
def lut_pair():
    if not _core.gpu_available():
        pytest.skip("no GPU")
    gpu, cpu = orc.make_pair(True)
    assert gpu.gpu_active
    return gpu, cpu


def k4_pair():
    if not _core.gpu_available():
        pytest.skip("no GPU")
    gpu, cpu = orc.make_pair(False, try_nots=True)
    assert gpu.gpu_active
    return gpu, cpu


@functools.lru_cache(maxsize=None)
def pool(n):
    """(state, tables) of the sentinel pool with n gates."""
    st = orc.cpu_engine(3).initial_state()
    st.grow_pool_random(n, 0x5E17 + n)
    assert st.num_gates == n
    return st, [st.gate(i)["table"] for i in range(n)]


def plant(k, tabs, rng, threes=None):
    """A target realised by the gates `tabs`, in this order, that is neither
    constant 0 (the mask needs a target-1 position) nor constant 1."""
    full = orc.tt_int(FULL)
    for _ in range(100):
        if k == 3:
            target = gen_lut_ttable(rng.randrange(1, 255), *tabs)
        elif k == 4:
            # Identity argument order, function from the available list.
            target = gen_lut_ttable(rng.choice(threes)["fun"], *tabs)
        elif k == 5:
            t_o = gen_lut_ttable(rng.randrange(1, 255), *tabs[:3])
            target = gen_lut_ttable(rng.randrange(1, 255), t_o, tabs[3],
                                    tabs[4])
        else:
            t_o = gen_lut_ttable(rng.randrange(1, 255), *tabs[:3])
            t_m = gen_lut_ttable(rng.randrange(1, 255), *tabs[3:6])
            target = gen_lut_ttable(rng.randrange(1, 255), t_o, t_m, tabs[6])
        if 0 < orc.tt_int(target) & full < full:
            orc.assert_mask_has_target1(target, FULL)
            return target
    raise AssertionError("no non-constant planted target")


def check_sentinel(gpu, cpu, k, n, comb, rng, threes=None):
    st, tabs = pool(n)
    kk = 3 if k == 4 else k
    comb = list(comb)
    assert len(comb) == kk and comb == sorted(set(comb)) and comb[-1] < n
    total = math.comb(n, kk)
    r = orc.checked_rank(comb, n)
    assert orc.checked_unrank(r, n, kk) == comb
    target = plant(k, [tabs[i] for i in comb], rng, threes)
    where = (k, n, comb, r)

    f_g, r_g, _ = gpu.scan_pool(k, st, target, FULL, r, r + 1, seed=SEED)
    f_c, r_c, _ = cpu.scan_pool(k, st, target, FULL, r, r + 1, seed=SEED)
    assert f_c, where
    assert f_g, where
    assert orc.hit_ids(k, r_g) == comb, (where, list(r_g))
    assert orc.hit_ids(k, r_c) == comb, (where, list(r_c))
    orc.assert_hit_valid(k, st, r_g, target, FULL, threes)

    a, b = max(0, r - 2000), min(total, r + 2001)
    f_g, r_g, _ = gpu.scan_pool(k, st, target, FULL, a, b, seed=SEED)
    f_c, r_c, _ = cpu.scan_pool(k, st, target, FULL, a, b, seed=SEED)
    assert f_c, (where, a, b)
    assert f_g, (where, a, b)
    orc.assert_hit_valid(k, st, r_g, target, FULL, threes)
    orc.assert_hit_valid(k, st, r_c, target, FULL, threes)
    hit_rank = orc.checked_rank(orc.hit_ids(k, r_g), n)
    assert a <= hit_rank < b, (where, a, b, list(r_g))


# --- k=3 and k=4 at pool 500 ------------------------------------------------

def triple_sentinels(n):
    total = math.comb(n, 3)
    combs = {tuple(orc.unrank(r, n, 3)) for r in (0, 1, total - 2, total - 1)}
    for a in (0, 1, 2, 250, 400, 495, 496, 497):
        # First and last triple of the block of a.
        combs.add((a, a + 1, a + 2))
        combs.add((a, n - 2, n - 1))
        # First and last triple of its rows b = a + 1 and b = n - 2.
        combs.add((a, a + 1, n - 1))
        for b in (a + 1, n - 2):
            combs.add((a, b, b + 1))
            combs.add((a, b, n - 1))
    rng = random.Random(0x500)
    combs |= {tuple(orc.unrank(rng.randrange(total), n, 3))
              for _ in range(200)}
    return sorted(combs)


def test_triple_sentinel_list():
    """The hand-built list holds the block and row boundaries it claims."""
    n = 500
    combs = triple_sentinels(n)
    ranks = sorted(orc.rank(c, n) for c in combs)
    total = math.comb(n, 3)
    assert {0, 1, total - 2, total - 1} <= set(ranks)
    for a in (0, 1, 2, 250, 400, 495, 496, 497):
        first = total - math.comb(n - a, 3)
        last = total - math.comb(n - a - 1, 3) - 1
        assert first in ranks and last in ranks
        assert orc.unrank(first, n, 3)[0] == a == orc.unrank(last, n, 3)[0]
        if first > 0:
            assert orc.unrank(first - 1, n, 3)[0] == a - 1
        # Row b = a + 1 spans [first, first + n - a - 2).
        assert first + n - a - 3 in ranks
    assert len(combs) >= 200


@gpu_test
def test_scan3_sentinels_pool500(lut_pair):
    gpu, cpu = lut_pair
    rng = random.Random(0x3500)
    for comb in triple_sentinels(500):
        check_sentinel(gpu, cpu, 3, 500, comb, rng)


@gpu_test
def test_scan4_service_sentinels_pool500(monkeypatch, capfd):
    monkeypatch.delenv("SBOXGATES_NO_SVC", raising=False)
    gpu, cpu = k4_pair()
    threes = orc.threes_default()
    rng = random.Random(0x4500)
    for comb in triple_sentinels(500):
        check_sentinel(gpu, cpu, 4, 500, comb, rng, threes)
    assert gpu.stats()["cpu_scans"] == 0
    # No fall-back from a failed service to the one-shot kernel.
    assert "scan service disabled" not in capfd.readouterr().err


@gpu_test
def test_scan4_oneshot_sentinels_pool500(monkeypatch):
    """The same on the one-shot k_scan4 kernel (see
    test_gpu_per_rank.test_scan4_oneshot_per_rank)."""
    monkeypatch.setenv("SBOXGATES_NO_SVC", "1")
    gpu, cpu = k4_pair()
    threes = orc.threes_default()
    rng = random.Random(0x4501)
    combs = triple_sentinels(500)
    for comb in combs:
        check_sentinel(gpu, cpu, 4, 500, comb, rng, threes)
    stats = gpu.stats()
    assert stats["gpu_scans"] == 2 * len(combs) and stats["cpu_scans"] == 0


# --- k=5 at pools 450, 500 and 90 -------------------------------------------

def quint_sentinels(n):
    combs = {tuple(range(5)), tuple(range(n - 5, n))}
    rng = random.Random(0x5000 + n)
    triples = [(0, 1, 2), (0, 1, n - 4), (0, 1, n - 3), (n - 5, n - 4, n - 3)]
    # c <= n - 3 leaves room for a pair behind the triple.
    triples += [tuple(sorted(rng.sample(range(n - 2), 3))) for _ in range(2)]
    for t in triples:
        c = t[2]
        for d, e in ((c + 1, c + 2), (c + 1, n - 1), (n - 2, n - 1)):
            assert c < d < e < n
            combs.add(t + (d, e))
    # Every position of a 16-pair row segment and both segment boundaries.
    combs |= {(0, 1, 2, 3, e) for e in range(4, 4 + 41)}
    return sorted(combs)


def row_sentinels_pool90():
    """Rows d = 3 and d = 60 of triple (0, 1, 2): e below and above id 64,
    and a short row."""
    n = 90
    combs = []
    for d in (3, 60):
        combs += [(0, 1, 2, d, e) for e in range(d + 1, min(n, d + 42))]
    assert any(c[4] < 64 for c in combs) and any(c[4] > 64 for c in combs)
    return combs


@gpu_test
@pytest.mark.parametrize("n", [450, 500, 90])
def test_scan5_sentinels(lut_pair, n):
    gpu, cpu = lut_pair
    rng = random.Random(0x5500 + n)
    combs = row_sentinels_pool90() if n == 90 else quint_sentinels(n)
    for comb in combs:
        check_sentinel(gpu, cpu, 5, n, comb, rng)


# --- k=7 at pools 40, 64 and 100 --------------------------------------------

def sept_sentinels(n):
    rng = random.Random(0x7000 + n)
    quads = [(0, 1, 2, 3), (0, 1, 2, n - 4),
             tuple(sorted(rng.sample(range(n - 8), 4)))]
    combs = set()
    for q in quads:
        d = q[3]
        e_mid = (d + 1 + n - 3) // 2   # an e-block in the middle
        for tail in ((d + 1, d + 2, d + 3), (n - 3, n - 2, n - 1),
                     (e_mid, e_mid + 1, e_mid + 2), (e_mid, n - 2, n - 1)):
            assert d < tail[0] < tail[1] < tail[2] < n
            combs.add(q + tail)
    return sorted(combs)


@gpu_test
@pytest.mark.parametrize("n", [40, 64, 100])
def test_scan7_sentinels(lut_pair, n):
    gpu, cpu = lut_pair
    rng = random.Random(0x7700 + n)
    for comb in sept_sentinels(n):
        check_sentinel(gpu, cpu, 7, n, comb, rng)


# --- k=7 exclusions at pool 70 ----------------------------------------------

@gpu_test
def test_scan7_exclusions_pool70(lut_pair):
    """Exclusion sets cover ids below 64 only; at pool 70 the tails reach
    ids 64..69, which no set may drop."""
    gpu, cpu = lut_pair
    n, w = 70, 200_000
    st, _ = pool(n)
    target = gpu.target(0)
    total = math.comb(n, 7)
    a_change = math.comb(n, 7) - math.comb(n - 1, 7)   # first rank with a = 1
    windows = [0, a_change - w // 2, total - w]
    six = 0
    for g in random.Random(0x70).sample(range(64), 6):
        six |= 1 << g
    sets = [1 << 63, 1 << 0 | 1 << 63, six]
    assert orc.unrank(a_change - 1, n, 7)[0] == 0
    assert orc.unrank(a_change, n, 7)[0] == 1

    # The last window in closed form: walk its combinations in Python.
    comb = orc.unrank(total - w, n, 7)
    it = itertools.dropwhile(lambda c: list(c) != comb,
                             itertools.combinations(range(comb[0], n), 7))
    last = [sum(1 << g for g in c if g < 64) for c in it]
    assert len(last) == w
    assert comb[0] >= 6   # so ids 0..5 are absent from the last window

    acted = False
    for excl in sets:
        for begin in windows:
            _, _, ev_g = gpu.scan_pool(7, st, target, FULL, begin, begin + w,
                                       count_all=True, excl=excl)
            _, _, ev_c = cpu.scan_pool(7, st, target, FULL, begin, begin + w,
                                       count_all=True, excl=excl)
            assert ev_g == ev_c, (hex(excl), begin, ev_g, ev_c)
            acted = acted or 0 < ev_c < w
            if begin == total - w:
                assert ev_g == sum(1 for m in last if not m & excl), hex(excl)
    assert acted
    # Ids 64..69 taken modulo 64 are 0..5: a set of exactly those ids must
    # leave the last window, which holds none of them, untouched.
    _, _, ev_g = gpu.scan_pool(7, st, target, FULL, total - w, total,
                               count_all=True, excl=0x3f)
    _, _, ev_c = cpu.scan_pool(7, st, target, FULL, total - w, total,
                               count_all=True, excl=0x3f)
    assert ev_g == ev_c == w
