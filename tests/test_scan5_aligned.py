"""k_scan5 wide walk (gfx950) at pools that are no multiple of its 64-gate
word groups, against cpu_scan5 and the independent oracle.

The walk aligns its word groups to the pool's end: inside it a gate has the
id gate + pad, pad = (64 - n % 64) % 64. These tests pin what a caller sees
(verdicts, results, evaluated counts), at the gate ids where that shift can
go wrong: both sides of every shifted 32-gate boundary (real id 32 k - pad)
and of every absolute one, the row's start, the pool's last gate, exclusion
sets on the ids that land on shifted bits 63 and 64, and the largest pool.
They hold for any layout of the groups.

Pools: 65 (pad 63), 127 (pad 1), 128 (pad 0); 70 for exclusion; 500
(MAX_GATES, pad 12).
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
POOLS = (65, 127, 128)


def pad_of(n):
    return (64 - n % 64) % 64


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
    st.grow_pool_random(n, 0xA11 + n)
    assert st.num_gates == n
    tabs = [st.gate(i)["table"] for i in range(n)]
    return st, tabs, [orc.tt_int(t) for t in tabs]


@functools.lru_cache(maxsize=None)
def aes_target():
    return orc.cpu_engine(5).target(0)


def plant(tabs, ids, rng):
    """A non-constant target that LUT(LUT(a, b, c), d, e) over the gates
    `ids` realises."""
    full = orc.tt_int(FULL)
    for _ in range(100):
        t_o = gen_lut_ttable(rng.randrange(1, 255), tabs[ids[0]], tabs[ids[1]],
                             tabs[ids[2]])
        target = gen_lut_ttable(rng.randrange(1, 255), t_o, tabs[ids[3]],
                                tabs[ids[4]])
        if 0 < orc.tt_int(target) & full < full:
            return target
    raise AssertionError("no non-constant planted target")


def edge_ids(n):
    """Real ids next to the shifted and the absolute 32-gate boundaries."""
    pad = pad_of(n)
    ids = set()
    for k in range(0, n + pad + 1, 32):
        for base in (k - pad, k):
            ids.update((base - 1, base, base + 1))
    return {i for i in ids if 0 <= i < n}


@functools.lru_cache(maxsize=None)
def boundary_combs(n):
    """Triple (0, 1, 2), and (0, 1, c) for the first shifted boundary c whose
    row still takes the wide walk, with d and e on both sides of every
    shifted and absolute 32-gate boundary, at the row's start and at the
    pool's last gate."""
    pad = pad_of(n)
    triples = [(0, 1, 2)]
    for k in range(32, n + pad, 32):
        c = k - pad
        if c > 2 and n - 1 - c > WIDE_MIN_ROW:
            triples.append((0, 1, c))
            break
    edges = edge_ids(n)
    out = []
    for a, b, c in triples:
        assert n - 1 - c > WIDE_MIN_ROW
        for d in sorted(edges | {c + 1, n - 2}):
            if d <= c or d > n - 2:
                continue
            for e in sorted(edges | {d + 1, n - 1}):
                if d < e < n:
                    out.append((a, b, c, d, e))
    assert len(out) >= 20
    return tuple(out)


@functools.lru_cache(maxsize=None)
def boundary_ranks(n):
    return tuple(orc.checked_rank(comb, n) for comb in boundary_combs(n))


def count_both(gpu, cpu, st, b, e, excl=0):
    target = aes_target()
    _, _, ev_g = gpu.scan_pool(5, st, target, FULL, b, e, seed=SEED,
                               count_all=True, excl=excl)
    _, _, ev_c = cpu.scan_pool(5, st, target, FULL, b, e, seed=SEED,
                               count_all=True, excl=excl)
    return ev_g, ev_c


def check_verdicts(gpu, cpu, n, combs, planted):
    """Single-rank windows: with a target planted on the combination (found,
    valid, res as the CPU's) and with the plain AES bit-0 target (verdict as
    the oracle's and the CPU's)."""
    st, tabs, ints = pool(n)
    rng = random.Random(0xA1 + n)
    aes = aes_target()
    t_int, m_int = orc.tt_int(aes), orc.tt_int(FULL)
    for comb in combs:
        r = orc.checked_rank(comb, n)
        assert orc.checked_unrank(r, n, 5) == list(comb)
        if planted:
            target = plant(tabs, comb, rng)
            f_g, r_g, ev_g = gpu.scan_pool(5, st, target, FULL, r, r + 1,
                                           seed=SEED)
            f_c, r_c, ev_c = cpu.scan_pool(5, st, target, FULL, r, r + 1,
                                           seed=SEED)
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
# 1. Verdicts at the shifted and absolute word boundaries.
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", POOLS)
def test_boundary_verdicts(engines, n):
    gpu, cpu = engines
    assert n - 3 > WIDE_MIN_ROW
    check_verdicts(gpu, cpu, n, boundary_combs(n), planted=True)


# ---------------------------------------------------------------------------
# 2. Window clipping.
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", POOLS)
def test_window_clipping(engines, n):
    """count_all windows that begin or end at a boundary rank or next to
    it, and the full range."""
    gpu, cpu = engines
    st, _, _ = pool(n)
    total = math.comb(n, 5)
    span = 1500
    windows = set()
    for r in boundary_ranks(n):
        for x in (r - 1, r, r + 1):
            if 0 <= x < total:
                windows.add((x, min(total, x + span)))
            if 0 < x <= total:
                windows.add((max(0, x - span), x))
    for b, e in sorted(windows):
        ev_g, ev_c = count_both(gpu, cpu, st, b, e)
        assert ev_g == e - b, (b, e, ev_g)
        assert ev_g == ev_c, (b, e, ev_g, ev_c)
    _, _, ev = gpu.scan_pool(5, st, aes_target(), FULL, 0, total, seed=SEED,
                             count_all=True)
    assert ev == total


# ---------------------------------------------------------------------------
# 3. Exclusion on the shifted edges, pools 65 and 70.
# ---------------------------------------------------------------------------
def bits(ids):
    out = 0
    for i in ids:
        assert 0 <= i < 64
        out |= 1 << i
    return out


def excl_sets(n):
    """The real ids that land on shifted bits 63 and 64, with ids 0 and
    63."""
    pad = pad_of(n)
    on_edge = {63 - pad, 64 - pad}
    return {
        "edges_0_63": sorted(on_edge | {0, 63}),
        "edges": sorted(on_edge),
        "low": [0],
        "high": [63],
    }


@pytest.mark.parametrize("which", ["edges_0_63", "edges", "low", "high"])
@pytest.mark.parametrize("n", [65, 70])
def test_exclusion_counts(engines, n, which):
    gpu, cpu = engines
    st, _, _ = pool(n)
    ids = excl_sets(n)[which]
    excl = bits(ids)
    total = math.comb(n, 5)
    ev_g, ev_c = count_both(gpu, cpu, st, 0, total, excl=excl)
    assert ev_g == ev_c, (n, which, ev_g, ev_c)
    assert ev_g == math.comb(n - len(ids), 5), (n, which, ev_g)
    rng = random.Random(excl & 0xFFFF)
    for _ in range(30):
        length = int(2 ** rng.uniform(0, 17))
        b = rng.randrange(0, total - length)
        ev_g, ev_c = count_both(gpu, cpu, st, b, b + length, excl=excl)
        assert ev_g == ev_c, (n, which, b, length, ev_g, ev_c)


# ---------------------------------------------------------------------------
# 4. The largest pool.
# ---------------------------------------------------------------------------
def test_pool_500(engines):
    """MAX_GATES gates (pad 12, top word full): the full range counts
    C(500, 5), and combinations that hold gates 0, 498 and 499 get the
    oracle's verdict."""
    n = _core.MAX_GATES
    assert n == 500
    gpu, cpu = engines
    st, _, _ = pool(n)
    total = math.comb(n, 5)
    _, _, ev = gpu.scan_pool(5, st, aes_target(), FULL, 0, total, seed=SEED,
                             count_all=True)
    assert ev == total
    middles = [(1, 2), (1, 497), (2, 250), (31, 32), (51, 52), (52, 53),
               (63, 64), (243, 244), (255, 256), (435, 436), (436, 437),
               (496, 497)]
    combs = [(0, x, y, 498, 499) for x, y in middles]
    check_verdicts(gpu, cpu, n, combs, planted=False)
