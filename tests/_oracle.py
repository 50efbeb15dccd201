"""Independent reference for the combination scans, shared by the oracle
tests: pure Python and numpy, written from the definition of each scan's
verdict. It takes truth tables as 256-bit integers built from
`state.gate(i)["table"]` and uses none of the engine's cell algebra (no
lut5_solve, no lut7_solve, no naive_* helper); the only engine functions it
calls are gen_lut_ttable / tt_eq_mask, to re-evaluate a reported hit, and
function_lists, for the list the k=4 result indexes.

Every mask used with it must hold at least one position where the target is
1 (sparse_mask asserts it): that excludes the engine's "function 00 does not
round-trip" special cases, so the oracle needs no knowledge of them.
"""

import functools
import itertools
import math
import random

import numpy as np

from sboxgates_amd import models
from sboxgates_amd.ops import (combination_rank, function_lists,
                               gen_lut_ttable, make_engine, nth_combination,
                               tt_eq_mask)

PERMS6 = [(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
# Gate set of the k=4 engines (the default: AND, OR, XOR) with try_nots.
GATE_BITFIELD = 2 + 64 + 128


# --- truth tables -----------------------------------------------------------

def tt_int(table: bytes) -> int:
    """256-bit truth table (4 little-endian u64) as an int; bit i = input i."""
    assert len(table) == 32
    return int.from_bytes(table, "little")


def tt_bytes(value: int) -> bytes:
    return value.to_bytes(32, "little")


def positions(mask: int):
    return [i for i in range(256) if (mask >> i) & 1]


def sparse_mask(seed, size, target: bytes) -> bytes:
    """Seeded mask of exactly `size` positions, at least one of them a
    target-1 position."""
    pos = random.Random(seed).sample(range(256), size)
    m = 0
    for p in pos:
        m |= 1 << p
    assert m & tt_int(target), "mask holds no target-1 position"
    return tt_bytes(m)


def assert_mask_has_target1(target: bytes, mask: bytes):
    assert tt_int(target) & tt_int(mask), "mask holds no target-1 position"


# --- combinations -----------------------------------------------------------

def unrank(r, n, k):
    """The k-combination of range(n) with lexicographic rank r."""
    assert 0 <= r < math.comb(n, k)
    out = []
    x = 0
    for j in range(k, 0, -1):
        # Combinations that start with x: C(n - x - 1, j - 1).
        while True:
            c = math.comb(n - x - 1, j - 1)
            if r < c:
                break
            r -= c
            x += 1
        out.append(x)
        x += 1
    return out


def rank(comb, n):
    """Inverse of unrank."""
    k = len(comb)
    r = 0
    prev = -1
    for j, c in enumerate(comb):
        for x in range(prev + 1, c):
            r += math.comb(n - x - 1, k - j - 1)
        prev = c
    return r


def checked_unrank(r, n, k):
    comb = unrank(r, n, k)
    assert comb == list(nth_combination(r, n, k)), (r, n, k)
    return comb


def checked_rank(comb, n):
    r = rank(comb, n)
    assert r == combination_rank(list(comb), n), (comb, n)
    return r


# --- cells and verdicts -----------------------------------------------------

def patterns(tabs, pos):
    """Input pattern of the ordered gate list at every position; the first
    gate is the most significant bit."""
    k = len(tabs)
    return [sum(((t >> p) & 1) << (k - 1 - j) for j, t in enumerate(tabs))
            for p in pos]


def cells(tabs, target, mask):
    """(patterns at masked target-1 positions, patterns at masked target-0
    positions) for an ordered list of gates."""
    pos = positions(mask)
    pat = patterns(tabs, pos)
    ones = {c for c, p in zip(pat, pos) if (target >> p) & 1}
    zeros = {c for c, p in zip(pat, pos) if not (target >> p) & 1}
    return ones, zeros


def found3(tabs, target, mask):
    ones, zeros = cells(tabs, target, mask)
    return not (ones & zeros)


def feasible7(tabs, target, mask):
    """Necessary condition for a 7-LUT hit: the 128 cells are disjoint."""
    ones, zeros = cells(tabs, target, mask)
    return not (ones & zeros)


def found4(tabs, target, mask, funs):
    """k=4 verdict: None, or (index into funs, argument-order index) of the
    first order, then first function, that realises the target. funs is the
    list of 8-bit function tables of function_lists(...)[2]."""
    for order, sel in enumerate(PERMS6):
        ones, zeros = cells([tabs[sel[0]], tabs[sel[1]], tabs[sel[2]]], target,
                            mask)
        if order == 0 and ones & zeros:
            return None
        for idx, fun in enumerate(funs):
            if (all((fun >> c) & 1 for c in ones)
                    and not any((fun >> c) & 1 for c in zeros)):
                return idx, order
    return None


_FO = np.arange(256, dtype=np.int64)


def found5(tabs, target, mask):
    """5-LUT verdict: some 3+2 split and some outer function among all 256
    leave no inner cell (o, d, e) with both target-1 and target-0 content."""
    pos = positions(mask)
    tgt = [(target >> p) & 1 for p in pos]
    for outer in itertools.combinations(range(5), 3):
        inner = [j for j in range(5) if j not in outer]
        po = patterns([tabs[j] for j in outer], pos)
        pi = patterns([tabs[j] for j in inner], pos)
        # Per inner pattern v: the outer patterns seen with target 1 / 0.
        a1 = [0] * 4
        a0 = [0] * 4
        for u, v, t in zip(po, pi, tgt):
            if t:
                a1[v] |= 1 << u
            else:
                a0[v] |= 1 << u
        bad = np.zeros(256, dtype=bool)
        for v in range(4):
            # Cell (o=1, v) collects the outer patterns where fo is 1.
            bad |= ((_FO & a1[v]) != 0) & ((_FO & a0[v]) != 0)
            bad |= ((~_FO & a1[v]) != 0) & ((~_FO & a0[v]) != 0)
        if not bad.all():
            return True
    return False


# --- re-evaluating a reported hit -------------------------------------------

def hit_ids(k, res):
    """Sorted gate ids a result names."""
    lo, cnt = {3: (1, 3), 4: (2, 3), 5: (2, 5), 7: (3, 7)}[k]
    return sorted(res[lo:lo + cnt])


def hit_table(k, st, res, threes=None):
    """Truth table of the LUT / gate arrangement a scan result describes."""
    def tab(i):
        return st.gate(i)["table"]
    if k == 3:
        return gen_lut_ttable(res[0], tab(res[1]), tab(res[2]), tab(res[3]))
    if k == 4:
        sel = PERMS6[res[1]]
        gids = [res[2], res[3], res[4]]
        return gen_lut_ttable(threes[res[0]]["fun"], tab(gids[sel[0]]),
                              tab(gids[sel[1]]), tab(gids[sel[2]]))
    if k == 5:
        t_o = gen_lut_ttable(res[0], tab(res[2]), tab(res[3]), tab(res[4]))
        return gen_lut_ttable(res[1], t_o, tab(res[5]), tab(res[6]))
    t_o = gen_lut_ttable(res[0], tab(res[3]), tab(res[4]), tab(res[5]))
    t_m = gen_lut_ttable(res[1], tab(res[6]), tab(res[7]), tab(res[8]))
    return gen_lut_ttable(res[2], t_o, t_m, tab(res[9]))


def assert_hit_valid(k, st, res, target, mask, threes=None):
    assert tt_eq_mask(target, hit_table(k, st, res, threes), mask), (k, res)


# --- engines and the per-rank cases -----------------------------------------

def rijndael_engine(lut_graph, gpu="off", **kw):
    sbox, n = models.load("rijndael")
    e = make_engine(lut_graph=lut_graph, seed=1, gpu=gpu, save_states=False,
                    **kw)
    e.set_sbox(sbox, n)
    return e


def make_pair(lut_graph, **kw):
    """(gpu="force", gpu="off") engines on the rijndael S-box."""
    return (rijndael_engine(lut_graph, gpu="force", **kw),
            rijndael_engine(lut_graph, **kw))


def threes_default():
    return function_lists(GATE_BITFIELD, True)[2]


# (k, pool, mask size) of the per-rank cases: single-rank windows over the
# whole combination space. Pools are grown with POOL_SEED + pool; the mask of
# a case is sparse_mask(MASK_SEED[case], size, target bit 0). The seeds are
# fixed; test_oracle.py asserts that every case has between 2% and 98% hits.
POOL_SEED = 0x77
SCAN_SEED = 7
PER_RANK_CASES = (
    [(3, 24, s) for s in (4, 6, 8)] +
    [(4, 24, s) for s in (4, 6, 8)] +
    [(5, 12, s) for s in (6, 8, 12, 16)] +
    [(7, 10, s) for s in (12, 16, 24)] +
    [(7, 11, s) for s in (12, 16, 24)])
MASK_SEED = {case: 1000 * case[0] + 10 * case[1] + case[2]
             for case in PER_RANK_CASES}
# The formula's mask for this case leaves 2 hits in 330 ranks (0.6%), below
# the 2% floor; this one leaves 36 (10.9%).
MASK_SEED[7, 11, 24] = 71124


def case_id(case):
    return "k%d-pool%d-mask%d" % case


@functools.lru_cache(maxsize=None)
def cpu_engine(k):
    return rijndael_engine(k != 4, **({"try_nots": True} if k == 4 else {}))


@functools.lru_cache(maxsize=None)
def case_setup(case):
    """(state, target, mask, total ranks) of a per-rank case."""
    k, pool, size = case
    eng = cpu_engine(k)
    st = eng.initial_state()
    st.grow_pool_random(pool, POOL_SEED + pool)
    assert st.num_gates == pool
    target = eng.target(0)
    mask = sparse_mask(MASK_SEED[case], size, target)
    return st, target, mask, math.comb(pool, 3 if k == 4 else k)


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """Per rank: (combination, oracle verdict, CPU found, CPU res). The
    oracle verdict is a bool for k=3/5, None or (function, order) for k=4,
    and the necessary condition for k=7. Computed once and shared."""
    k, pool, size = case
    st, target, mask, total = case_setup(case)
    eng = cpu_engine(k)
    tabs = [tt_int(st.gate(i)["table"]) for i in range(pool)]
    t, m = tt_int(target), tt_int(mask)
    funs = [f["fun"] for f in threes_default()] if k == 4 else None
    kk = 3 if k == 4 else k
    out = []
    for r in range(total):
        comb = checked_unrank(r, pool, kk)
        g = [tabs[i] for i in comb]
        if k == 3:
            verdict = found3(g, t, m)
        elif k == 4:
            verdict = found4(g, t, m, funs)
        elif k == 5:
            verdict = found5(g, t, m)
        else:
            verdict = feasible7(g, t, m)
        f_c, r_c, _ = eng.scan_pool(k, st, target, mask, r, r + 1,
                                    seed=SCAN_SEED)
        out.append((comb, verdict, f_c, tuple(r_c)))
    return tuple(out)
