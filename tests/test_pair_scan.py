"""The pair scan (k=2) of gate-mode steps 3 and 4a on the CPU, against the
independent oracle of tests/_oracle_pairs.py: per-rank verdicts and result
words, the lowest-rank hit and the `evaluated` count of wider windows, the
matcher table, the edge cases, and the engine wiring on planted targets.

Cases: gate set 214 with try_nots (both lists hold non-commutative
functions), Rijndael bit 0, pool 24, sparse masks of 3, 4 and 5 positions.
Oracle hits out of 276 ranks (gates list, of them swapped; NOT list, of them
swapped): mask 3: 140, 28; 45, 19. Mask 4: 16, 2; 7, 4. Mask 5: 10, 6; 11, 0.
"""

import math

import pytest

import _oracle as orc
import _oracle_pairs as op
from sboxgates_amd import _core
from sboxgates_amd.ops import (function_lists, gen_ttable_2, make_engine,
                               pair2_matcher, scan_pairs)

CASES = [(s, w) for s in op.MASK_SIZES for w in op.LISTS]
COUNTS = {(3, "gates"): (140, 28), (3, "not"): (45, 19),
          (4, "gates"): (16, 2), (4, "not"): (7, 4),
          (5, "gates"): (10, 6), (5, "not"): (11, 0)}


def case_id(case):
    return "mask%d-%s" % case


def test_oracle_evaluates_functions_like_gen_ttable_2():
    eng = op.cpu_engine()
    st = eng.initial_state()
    st.grow_pool_random(12, 3)
    for fun in range(16):
        for a, b in ((8, 9), (11, 10), (3, 7)):
            ta, tb = st.gate(a)["table"], st.gate(b)["table"]
            assert (op.fun2_table(fun, orc.tt_int(ta), orc.tt_int(tb)) ==
                    orc.tt_int(gen_ttable_2(fun, ta, tb))), fun


def test_case_lists_hold_non_commutative_functions():
    lists = op.fun_lists()
    for which in op.LISTS:
        assert any(not f["ab_commutative"] for f in lists[which]), which
        assert len(lists[which]) <= 48


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_oracle_hit_counts(case):
    size, which = case
    v = op.case_verdicts(size, which, "identity")
    assert len(v) == op.TOTAL == 276
    hits = sum(x is not None for x in v)
    swapped = sum(1 for x in v if x is not None and x[1])
    assert (hits, swapped) == COUNTS[case]
    # The band tests/test_oracle.py holds its cases to.
    assert 0.02 * op.TOTAL <= hits <= 0.98 * op.TOTAL


@pytest.mark.parametrize("size", op.MASK_SIZES)
def test_every_mask_size_has_a_swapped_hit(size):
    assert any(x is not None and x[1]
               for which in op.LISTS
               for x in op.case_verdicts(size, which, "identity"))


def check_per_rank(eng, size, which, order_name):
    """Single-rank windows over all ranks on `eng`; returns the scan count."""
    st, target, mask = op.case_setup(size)
    orc.assert_mask_has_target1(target, mask)
    funs = op.fun_lists()[which]
    order = op.orders(op.POOL)[order_name]
    verdicts = op.case_verdicts(size, which, order_name)
    for r, verdict in enumerate(verdicts):
        found, res, ev = scan_pairs(eng, st, target, mask, r, r + 1, which,
                                    None if order_name == "identity" else order)
        where = (size, which, order_name, r)
        assert ev == 1, where
        assert found == (verdict is not None), where
        if not found:
            assert list(res) == [0] * 10, where
            continue
        i, k = op.pair_of_rank(r, op.POOL)
        assert tuple(res[:4]) == op.expected(verdict, order[i], order[k]), where
        assert list(res[4:]) == [0] * 6, where
        op.assert_hit_valid(st, funs, res, target, mask)
    return len(verdicts)


@pytest.mark.parametrize("order_name", ["identity", "reversed", "shuffled"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_cpu_per_rank(case, order_name):
    eng = op.rijndael_engine()
    scans = check_per_rank(eng, case[0], case[1], order_name)
    stats = eng.stats()
    assert stats["pair_scans_cpu"] == scans and stats["pair_scans_gpu"] == 0
    # Pair scans keep out of the counters of the other scans.
    assert stats["cpu_scans"] == 0 and stats["gpu_scans"] == 0


def windows(verdicts):
    first = next(r for r, v in enumerate(verdicts) if v is not None)
    return [(0, 276), (17, 200), (first + 1, 276), (first, first + 1),
            (0, first), (100, 101), (275, 276), (250, 1000)]


@pytest.mark.parametrize("order_name", ["identity", "shuffled"])
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_cpu_windows_lowest_rank_and_evaluated(case, order_name):
    size, which = case
    eng = op.cpu_engine()
    st, target, mask = op.case_setup(size)
    order = op.orders(op.POOL)[order_name]
    verdicts = op.case_verdicts(size, which, order_name)
    for begin, end in windows(verdicts):
        f_r, res_r, ev_r = op.window_reference(verdicts, order, begin, end)
        found, res, ev = scan_pairs(eng, st, target, mask, begin, end, which,
                                    order)
        where = (case, order_name, begin, end)
        assert (found, ev) == (f_r, ev_r), where
        if found:
            assert tuple(res[:4]) == res_r, where


@pytest.mark.parametrize("bitfield", [214, 194, 65535, 2 + 4])
@pytest.mark.parametrize("which", op.LISTS)
def test_matcher_table(bitfield, which):
    funs = dict(zip(op.LISTS, function_lists(bitfield, True)[:2]))[which]
    table = pair2_matcher(bitfield, True, which)
    assert len(table) == 256

    def satisfies(fun, care, req1, swap):
        # Pattern p = a << 1 | b; swapped, the function sees (b, a).
        for p in range(4):
            if not (care >> p) & 1:
                continue
            a, b = p >> 1, p & 1
            if op.fun2(fun, b, a) if swap else op.fun2(fun, a, b):
                if not (req1 >> p) & 1:
                    return False
            elif (req1 >> p) & 1:
                return False
        return True

    for care in range(16):
        for req1 in range(16):
            want = 0xFF
            if req1 & ~care == 0:
                for m, f in enumerate(funs):
                    if satisfies(f["fun"], care, req1, False):
                        want = m
                        break
                    if not f["ab_commutative"] and satisfies(f["fun"], care,
                                                             req1, True):
                        want = m | 0x80
                        break
            assert table[care << 4 | req1] == want, (care, req1)


def test_edge_cases():
    eng = op.cpu_engine()
    st, target, mask = op.case_setup(3)
    # begin at or past the total: nothing examined.
    for begin in (276, 277, 10 ** 6):
        assert scan_pairs(eng, st, target, mask, begin, begin + 5)[::2] == (
            False, 0)
    # An empty window.
    assert scan_pairs(eng, st, target, mask, 5, 5)[::2] == (False, 0)
    # end past the total is clipped: a miss window counts up to the total.
    verdicts = op.case_verdicts(5, "gates", "identity")
    last = max(r for r, v in enumerate(verdicts) if v is not None)
    st5, target5, mask5 = op.case_setup(5)
    found, _, ev = scan_pairs(eng, st5, target5, mask5, last + 1, 10 ** 9)
    assert (found, ev) == (False, 276 - last - 1)
    # Pools too small to hold a pair.
    sbox, _ = _core.load_sbox_table([0, 1], 0)
    tiny = make_engine(gpu="off", seed=1)
    tiny.set_sbox(sbox, 1)
    st1 = tiny.initial_state()
    assert st1.num_gates == 1
    assert scan_pairs(tiny, st1, tiny.target(0), mask, 0, 10)[::2] == (False, 0)
    # A bad order or list name is refused.
    with pytest.raises(ValueError):
        scan_pairs(eng, st, target, mask, 0, 276, order=[0] * 24)
    with pytest.raises(ValueError):
        scan_pairs(eng, st, target, mask, 0, 276, order=list(range(23)))
    with pytest.raises(ValueError):
        scan_pairs(eng, st, target, mask, 0, 276, funs="luts")


@pytest.mark.parametrize("n", [200, 500])
def test_big_pools_have_hits_past_rank_0(n):
    """What the GPU election tests rely on: under the shuffled order both
    large pools have at least 3 hits and none at rank 0."""
    eng = op.cpu_engine()
    st, target, mask, order = op.big_pool(n)
    assert n <= _core.MAX_GATES
    for which in op.LISTS:
        hits = op.cpu_hits(eng, st, target, mask, which, list(order), 3)
        assert len(hits) == 3 and hits[0] > 0, (n, which, hits)


@pytest.mark.parametrize("which", op.LISTS)
def test_engine_wiring_planted(which):
    """create_circuit finds a target that only a pair realises: through the
    gates list in step 3, through the NOT list (NOR of two gates) in step
    4a, the same under every gpu_pairs value of an engine without a GPU."""
    st, target, mask, m, pair = op.planted(which)
    t = orc.tt_int(target)
    full = (1 << 256) - 1
    for i in range(st.num_gates):
        g = orc.tt_int(st.gate(i)["table"])
        assert t != g and t != g ^ full
    xml = set()
    for gpu_pairs in ("off", "auto", "force"):
        eng = op.rijndael_engine(gpu_pairs=gpu_pairs)
        xml.add(op.check_planted_circuit(eng, which).to_xml())
        stats = eng.stats()
        assert stats["pair_scans_gpu"] == 0 and stats["pair_scans_cpu"] == 0
    assert len(xml) == 1


def test_options_gpu_pairs_property():
    o = _core.Options()
    assert o.gpu_pairs == "off"
    for v in ("auto", "force", "off"):
        o.gpu_pairs = v
        assert o.gpu_pairs == v
    with pytest.raises(ValueError):
        o.gpu_pairs = "on"
