"""Independent reference for the pair scan (k=2) of gate-mode steps 3 and
4a, shared by the pair-scan tests: pure Python, written from the scan's
definition. It evaluates each 2-input function position by position with
the 4-bit encoding documented in sbg/boolfunc.hpp (function bit 3 - p is the
output at pattern p = A << 1 | B) and compares under the mask, per list
entry, direct then swapped; it uses none of the engine's cell algebra and no
matcher table. The only engine functions it calls are gen_ttable_2, to
cross-check its evaluation of all 16 functions and to re-evaluate a reported
hit, tt_eq_mask, and function_lists, for the lists the result indexes.
"""

import functools
import math
import random

import _oracle as orc
from sboxgates_amd.ops import (function_lists, gen_ttable_2, make_engine,
                               tt_eq_mask)
from sboxgates_amd import models

# Gate set of the pair-scan cases: AND, both ANDN orders, XOR, OR. With
# try_nots both of its lists hold non-commutative functions.
GATE_BITFIELD = 214
LISTS = ("gates", "not")
POOL = 24
MASK_SIZES = (3, 4, 5)
TOTAL = math.comb(POOL, 2)


def fun2(fun, a, b):
    """Value of 2-input function `fun` at inputs a, b."""
    return (fun >> (3 - ((a << 1) | b))) & 1


def fun2_table(fun, ta, tb):
    """256-bit table of fun applied to two 256-bit tables, per position."""
    out = 0
    for p in range(256):
        out |= fun2(fun, (ta >> p) & 1, (tb >> p) & 1) << p
    return out


def realises(fun, tx, ty, target, mask_positions):
    return all(fun2(fun, (tx >> p) & 1, (ty >> p) & 1) == (target >> p) & 1
               for p in mask_positions)


def pair_verdict(tx, ty, target, mask_positions, funs):
    """None, or (index into funs, swapped) of the first list entry that
    realises the target under the mask, direct before swapped; a commutative
    entry is not tried swapped."""
    for m, f in enumerate(funs):
        if realises(f["fun"], tx, ty, target, mask_positions):
            return m, 0
        if not f["ab_commutative"] and realises(f["fun"], ty, tx, target,
                                                mask_positions):
            return m, 1
    return None


def pair_of_rank(r, n):
    """Visit positions (i, k), i < k, of rank r: row-major."""
    i, k = orc.unrank(r, n, 2)
    return i, k


def expected(verdict, x, y):
    """Result words (res[0..3]) of a hit at gates x = order[i], y = order[k]."""
    m, swapped = verdict
    return (m, swapped, y, x) if swapped else (m, swapped, x, y)


def window_reference(verdicts, order, begin, end):
    """(found, res[0..3], evaluated) of a window from the per-rank verdicts
    under `order` (a list indexed by rank)."""
    n = len(order)
    end = min(end, math.comb(n, 2))
    if begin >= end:
        return False, None, 0
    for r in range(begin, end):
        if verdicts[r] is not None:
            i, k = pair_of_rank(r, n)
            return True, expected(verdicts[r], order[i], order[k]), r - begin + 1
    return False, None, end - begin


def hit_table(st, funs, res):
    """Truth table of the function a result names, on its gates in argument
    order."""
    return gen_ttable_2(funs[res[0]]["fun"], st.gate(res[2])["table"],
                        st.gate(res[3])["table"])


def assert_hit_valid(st, funs, res, target, mask):
    assert tt_eq_mask(target, hit_table(st, funs, res), mask), res


# --- engines and cases -------------------------------------------------------

def fun_lists(bitfield=GATE_BITFIELD):
    gates, nots, _ = function_lists(bitfield, True)
    return {"gates": gates, "not": nots}


def rijndael_engine(gpu="off", bitfield=GATE_BITFIELD, **kw):
    sbox, n = models.load("rijndael")
    e = make_engine(lut_graph=False, seed=1, gpu=gpu, save_states=False,
                    try_nots=True, gate_bitfield=bitfield, **kw)
    e.set_sbox(sbox, n)
    return e


@functools.lru_cache(maxsize=None)
def cpu_engine(bitfield=GATE_BITFIELD):
    return rijndael_engine(bitfield=bitfield)


def orders(n, seed=0x0DE5):
    """Identity, reversed and one seeded shuffle."""
    shuffled = list(range(n))
    random.Random(seed + n).shuffle(shuffled)
    return {"identity": list(range(n)), "reversed": list(range(n - 1, -1, -1)),
            "shuffled": shuffled}


@functools.lru_cache(maxsize=None)
def case_setup(size):
    """(state, target, mask) of the pool-24 case with a mask of `size`."""
    eng = cpu_engine()
    st = eng.initial_state()
    st.grow_pool_random(POOL, orc.POOL_SEED + POOL)
    assert st.num_gates == POOL
    target = eng.target(0)
    mask = orc.sparse_mask(2000 + 10 * POOL + size, size, target)
    return st, target, mask


def pool_verdicts(st, target, mask, funs, order):
    """Oracle verdict of every rank of C(n, 2) under `order`."""
    n = st.num_gates
    tabs = [orc.tt_int(st.gate(i)["table"]) for i in range(n)]
    t = orc.tt_int(target)
    pos = orc.positions(orc.tt_int(mask))
    out = []
    for i in range(n):
        for k in range(i + 1, n):
            out.append(pair_verdict(tabs[order[i]], tabs[order[k]], t, pos, funs))
    return out


@functools.lru_cache(maxsize=None)
def case_verdicts(size, which, order_name):
    """Per-rank oracle verdicts of a pool-24 case, computed once."""
    st, target, mask = case_setup(size)
    order = orders(POOL)[order_name]
    return tuple(pool_verdicts(st, target, mask, fun_lists()[which], order))


@functools.lru_cache(maxsize=None)
def big_pool(n):
    """(state, target, mask, shuffled order) for the election tests on pools
    of 200 and 500 gates: Rijndael bit 0 under a 5-position mask."""
    eng = cpu_engine()
    st = eng.initial_state()
    st.grow_pool_random(n, orc.POOL_SEED + n)
    assert st.num_gates == n
    target = eng.target(0)
    mask = orc.sparse_mask(2000 + 10 * n + 5, 5, target)
    return st, target, mask, tuple(orders(n)["shuffled"])


def cpu_hits(eng, st, target, mask, which, order, limit):
    """Ranks of the first `limit` hits of the whole window on `eng`, found by
    restarting the scan just after each hit."""
    total = math.comb(st.num_gates, 2)
    hits = []
    begin = 0
    while begin < total and len(hits) < limit:
        found, _, ev = eng.scan_pairs(st, target, mask, begin, total, which,
                                      order)
        if not found:
            break
        hits.append(begin + ev - 1)
        begin += ev
    return hits


# --- planted targets for the engine-wiring tests -----------------------------

def planted(which):
    """(state, target, full mask, function index, {x, y}): a target that only
    one pair of the pool realises, through list `which` and not through the
    gates list when `which` is "not", and that no gate or complement of a
    gate equals (so steps 1 and 2 miss)."""
    eng = cpu_engine()
    st = eng.initial_state()
    st.grow_pool_random(POOL, orc.POOL_SEED + POOL)
    n = st.num_gates
    lists = fun_lists()
    full = (1 << 256) - 1
    pos = list(range(256))
    tabs = [orc.tt_int(st.gate(i)["table"]) for i in range(n)]
    # ANDN of two gates through the gates list; NOR through the NOT list.
    fun = 2 if which == "gates" else 8
    assert fun in [f["fun"] for f in lists[which]]
    rng = random.Random(0x9A1 + fun)
    for _ in range(200):
        x, y = rng.sample(range(n), 2)
        t = fun2_table(fun, tabs[x], tabs[y])
        if any(t == g or t == g ^ full for g in tabs):
            continue
        hits = {}
        for name in LISTS:
            hits[name] = [(i, k, pair_verdict(tabs[i], tabs[k], t, pos,
                                              lists[name]))
                          for i in range(n) for k in range(i + 1, n)]
            hits[name] = [h for h in hits[name] if h[2] is not None]
        mine = hits[which]
        if len(mine) != 1 or {mine[0][0], mine[0][1]} != {x, y}:
            continue
        if which == "not" and hits["gates"]:
            continue
        return st, orc.tt_bytes(t), orc.tt_bytes(full), mine[0][2][0], {x, y}
    raise AssertionError("no planted target found")


def check_planted_circuit(eng, which):
    """create_circuit on the planted state must append exactly the function
    the oracle predicts on the planted pair; returns the state."""
    st, target, mask, m, pair = planted(which)
    st = st.copy()
    n = st.num_gates
    f = fun_lists()[which][m]
    out = eng.create_circuit(st, target, mask)
    assert out == st.num_gates - 1
    assert tt_eq_mask(target, st.gate(out)["table"], mask)
    g = st.gate(out)
    if f["not_out"]:
        assert g["type_name"] == "NOT", g
        g = st.gate(g["in1"])
    assert g["type"] == f["fun1"], (g, f)
    assert not f["not_a"] and not f["not_b"]
    assert {g["in1"], g["in2"]} == pair, (g, pair)
    assert st.num_gates == n + 1 + (1 if f["not_out"] else 0)
    return st
