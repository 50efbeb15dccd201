"""The independent oracle of tests/_oracle.py against the CPU scans, on
single-rank windows [r, r+1) for every rank of the per-rank cases that
tests/test_gpu_per_rank.py runs on the GPU. Runs without a GPU, so the
oracle is kept honest in the suite that runs everywhere.

Likewise the CPU references of tests/test_gpu_onesided_masks.py (the CPU
scans on one-sided masks: hits valid, no zero function byte, the k=3 rule)
and of tests/test_gpu_large_pools.py (the share of windows that hold a
second hit, the rows that hit by their last rank)."""

import itertools
import math
import random

import pytest

import _oracle as orc
import _oracle_large as lg
import _oracle_onesided as one
import test_gpu_sentinels as sen
from conftest import rand_sparse_tt, rand_tt


def test_unranker_round_trip():
    rng = random.Random(5)
    for n, k in [(5, 3), (24, 3), (12, 5), (11, 7), (500, 3), (500, 5),
                 (100, 7)]:
        total = math.comb(n, k)
        ranks = {0, 1, total - 2, total - 1}
        ranks |= {rng.randrange(total) for _ in range(50)}
        for r in ranks:
            comb = orc.checked_unrank(r, n, k)
            assert comb == sorted(set(comb)) and comb[-1] < n
            assert orc.checked_rank(comb, n) == r
    assert [orc.unrank(r, 4, 2) for r in range(6)] == [
        [0, 1], [0, 2], [0, 3], [1, 2], [1, 3], [2, 3]]


def test_cells_order_and_verdicts_by_hand():
    """First gate is the most significant pattern bit; verdicts on a
    hand-made instance."""
    a, b, c = 0b1100, 0b1010, 0b0110
    ones, zeros = orc.cells([a, b, c], 0b1000, 0b1111)
    # Positions 0..3 carry patterns (a,b,c) = 000, 011, 101, 110.
    assert ones == {0b110} and zeros == {0b000, 0b011, 0b101}
    assert orc.found3([a, b, c], 0b1000, 0b1111)
    # a alone cannot tell position 2 from 3.
    assert not orc.found3([a, a, a], 0b1000, 0b1111)
    # AND(a, b) with c ignored is function 0xC0; it fits in the identity
    # order. 0x11 is 1 on pattern 000, a target-0 cell in every order.
    assert orc.found4([a, b, c], 0b1000, 0b1111, [0x11, 0xC0]) == (1, 0)
    assert orc.found4([a, b, c], 0b1000, 0b1111, [0x11]) is None

    # k=7 on the seven input variables x0..x6 themselves, full mask: every
    # cell holds exactly the two positions that differ in x7 alone, on which
    # both targets below agree, so both are feasible.
    x = [sum(1 << i for i in range(256) if (i >> j) & 1) for j in range(7)]
    full = (1 << 256) - 1
    # AND(x0,x1,x2) ^ OR(x3,x4,x5) ^ x6 is a 7-LUT by construction: fo = 80,
    # fm = fe, fi = 96. In that arrangement fm must tell pattern 000 from
    # the seven others, which only OR (fe) and NOR (01) do.
    t = 0
    for i in range(256):
        b = [(i >> j) & 1 for j in range(7)]
        t |= ((b[0] & b[1] & b[2]) ^ (b[3] | b[4] | b[5]) ^ b[6]) << i
    assert orc.feasible7(x, t, full) and orc.found7(x, t, full)
    assert ((0, 1, 2), (3, 4, 5), 6, 2) in orc.solvable_orderings7(x, t, full)
    assert orc.found7_naive(x, t, full, funs=(0x80, 0xFE, 0x01))
    # Majority of the seven is feasible but no 7-LUT. Fix the outer triple's
    # inputs at weight s: what remains is "at least 4 - s of the other four
    # are 1", a different function of those four for each s = 0..3. fo maps
    # the outer patterns to one bit, so two of the four weights share a
    # value of fo, and fi(fo, ., .) is then the same function of the other
    # four inputs for both. The target is symmetric, so that holds for every
    # arrangement.
    maj = sum(1 << i for i in range(256) if bin(i & 127).count("1") >= 4)
    assert orc.feasible7(x, maj, full)
    assert not orc.found7(x, maj, full)
    assert orc.solvable_orderings7(x, maj, full) == []


def test_arrangements7_are_the_70_classes():
    """The oracle's own enumeration: 140 ordered (outer, middle, leftover)
    arrangements, of which it keeps one per outer/middle swap."""
    keys = {(frozenset([o, m]), g) for o, m, g in orc.ARRANGEMENTS7_ALL}
    assert len(keys) == 70
    assert {(frozenset([o, m]), g) for o, m, g in orc.ARRANGEMENTS7} == keys
    for o, m, g in orc.ARRANGEMENTS7_ALL:
        assert sorted(o + m + (g,)) == list(range(7))


def test_found7_matches_naive_formulation():
    """found7 against found7_naive, which builds the three LUT tables and
    derives fi position by position. The naive form costs about 15 us per
    (arrangement, fo, fm), so it runs with fo and fm drawn from a random set
    of 10 function bytes (byte 00 always among them) on masks of up to 24
    positions, where both verdicts occur, and with all 256 on masks of up
    to 12 positions that found7 calls solvable."""
    rng = random.Random(7007)
    verdicts = []
    for _ in range(24):
        tabs = [orc.tt_int(rand_tt(rng)) for _ in range(7)]
        target = orc.tt_int(rand_tt(rng))
        mask = orc.tt_int(rand_sparse_tt(rng, rng.choice([8, 12, 16, 24])))
        funs = [0] + rng.sample(range(1, 256), 9)
        want = orc.found7_naive(tabs, target, mask, funs)
        assert orc.found7(tabs, target, mask, funs) == want
        assert bool(orc.solvable_orderings7(tabs, target, mask, funs)) == want
        verdicts.append(want)
    print("restricted function set: %d solvable, %d not"
          % (verdicts.count(True), verdicts.count(False)))
    assert verdicts.count(True) >= 5 and verdicts.count(False) >= 5
    full = 0
    for _ in range(6):
        tabs = [orc.tt_int(rand_tt(rng)) for _ in range(7)]
        target = orc.tt_int(rand_tt(rng))
        mask = orc.tt_int(rand_sparse_tt(rng, rng.choice([8, 12])))
        if orc.found7(tabs, target, mask):
            full += 1
            assert orc.found7_naive(tabs, target, mask)
    assert full >= 3


@pytest.mark.parametrize("case", orc.PER_RANK_CASES, ids=orc.case_id)
def test_oracle_matches_cpu_scan_per_rank(case):
    k, pool, size = case
    st, target, mask, total = orc.case_setup(case)
    orc.assert_mask_has_target1(target, mask)
    threes = orc.threes_default() if k == 4 else None
    hits = 0
    for r, (comb, verdict, f_c, r_c) in enumerate(orc.case_reference(case)):
        if k == 7:
            assert f_c == verdict.solvable, (r, comb)
            assert verdict.feasible or not f_c, (r, comb)  # found => feasible
            assert verdict.feasible or not verdict.solvable, (r, comb)
        elif k == 4:
            assert f_c == (verdict is not None), (r, comb)
            if f_c:
                assert (r_c[0], r_c[1]) == verdict, (r, comb, r_c, verdict)
        else:
            assert f_c == verdict, (r, comb)
        if f_c:
            hits += 1
            assert orc.hit_ids(k, r_c) == comb, (r, r_c)
            orc.assert_hit_valid(k, st, r_c, target, mask, threes)
    # A case must not pass vacuously. The oracle's verdicts equal the CPU's
    # (asserted above), so this is the share under the oracle.
    share = hits / total
    line = f"{orc.case_id(case)}: {hits}/{total} hits ({100 * share:.1f}%)"
    if k == 7:
        line += ("; %d feasible-unsolvable, %d solvable, %d in one arrangement"
                 ", %d of those with two fm" % k7_counts([case]))
    print(line)
    assert 0.02 <= share <= 0.98, share


K7_CASES = [c for c in orc.PER_RANK_CASES if c[0] == 7]


def k7_counts(cases):
    """Over the ranks of the cases, under the oracle alone: (feasible but
    unsolvable, solvable, solvable in exactly one arrangement, of those the
    ones whose arrangement admits only an fm and its complement)."""
    v = [verdict for case in cases
         for _, verdict, _, _ in orc.case_reference(case)]
    return (sum(x.feasible and not x.solvable for x in v),
            sum(x.solvable for x in v),
            sum(len(x.arrangements) == 1 for x in v),
            sum(x.tight_fm for x in v))


def test_k7_cases_tell_solvable_from_feasible():
    """Taken together the k=7 cases must be able to tell a correct solver
    from one that answers "feasible", from one that loses an arrangement,
    and from one that loses part of the fm sweep: counted under the oracle
    alone."""
    unsolvable, solvable, single, tight = k7_counts(K7_CASES)
    print("k=7 cases: %d feasible-unsolvable, %d solvable, %d in one "
          "arrangement, %d of those with two fm"
          % (unsolvable, solvable, single, tight))
    assert unsolvable >= 20
    assert solvable >= 20
    assert single >= 10
    assert tight >= 1


def test_deep_hit_list_instance():
    """The facts that the GPU test of the deep, mostly unsolvable hit list
    (test_gpu_per_rank.py) builds on, from the oracle and the CPU scan."""
    st, target, mask = orc.deep7_setup()
    orc.assert_mask_has_target1(target, mask)
    n = orc.DEEP7_POOL
    tabs = [orc.tt_int(st.gate(i)["table"]) for i in range(n)]
    t, m = orc.tt_int(target), orc.tt_int(mask)
    assert orc.checked_unrank(orc.DEEP7_FIRST, n, 7) == orc.DEEP7_COMB
    # itertools.combinations walks the combinations in rank order.
    feasible = [r for r, comb in enumerate(itertools.islice(
        itertools.combinations(range(n), 7), orc.DEEP7_FIRST))
        if orc.feasible7([tabs[i] for i in comb], t, m)]
    assert len(feasible) == orc.DEEP7_FEASIBLE
    assert orc.found7([tabs[i] for i in orc.DEEP7_COMB], t, m)
    for r in random.Random(36).sample(feasible, 40):
        comb = orc.checked_unrank(r, n, 7)
        assert not orc.found7([tabs[i] for i in comb], t, m), (r, comb)
    eng = orc.cpu_engine(7)
    (a0, b0), (a1, b1) = orc.DEEP7_WINDOWS
    f_c, _, ev = eng.scan_pool(7, st, target, mask, a0, b0, seed=orc.SCAN_SEED)
    assert not f_c and ev == orc.DEEP7_FIRST
    f_c, r_c, ev = eng.scan_pool(7, st, target, mask, a1, b1,
                                 seed=orc.SCAN_SEED)
    assert f_c and orc.hit_ids(7, r_c) == orc.DEEP7_COMB
    orc.assert_hit_valid(7, st, r_c, target, mask)


# --- one-sided masks --------------------------------------------------------

def test_onesided_masks_are_one_sided():
    target = orc.cpu_engine(3).target(0)
    t = orc.tt_int(target)
    full = (1 << 256) - 1
    masks = {n: orc.tt_int(m)
             for n, m in orc.onesided_masks(target, one.MASK_SEED).items()}
    assert list(masks) == list(orc.ONESIDED)
    sizes = {n: bin(m).count("1") for n, m in masks.items()}
    zeros = 256 - bin(t).count("1")
    assert sizes == {"Z1": 1, "Z6": 6, "Z40": 40, "Zall": zeros, "O1": 1,
                     "O40": 40, "Oall": 256 - zeros, "E": 0}
    for name, m in masks.items():
        assert not m & (t if name[0] == "Z" else ~t & full), name
    # A 6-input target: positions below 64 only.
    des = orc.tt_int(orc.tt_bytes(t & (1 << 64) - 1))
    for m in orc.onesided_masks(orc.tt_bytes(des), 1, 6).values():
        assert orc.tt_int(m) < 1 << 64


@pytest.mark.parametrize("name", orc.ONESIDED)
@pytest.mark.parametrize("kind", one.KINDS, ids=one.kind_id)
def test_cpu_scans_on_onesided_masks(kind, name):
    """What the GPU tests on one-sided masks take from the CPU scans: every
    hit names its rank's combination, realises the target under the mask
    and holds no zero function byte; cpu_scan3 follows found3_onesided on
    every rank; and the masks that have to give both answers do."""
    st, target, masks, total = one.setup(kind)
    mask = masks[name]
    ref = one.reference(kind, name)
    assert len(ref) == total
    tabs = [orc.tt_int(st.gate(i)["table"]) for i in range(st.num_gates)]
    t, m = orc.tt_int(target), orc.tt_int(mask)
    hits = 0
    for r, (comb, f_c, r_c, ev_c) in enumerate(ref):
        assert ev_c == 1, (r, comb)
        if kind == 3:
            assert f_c == orc.found3_onesided([tabs[i] for i in comb], t, m), \
                (r, comb)
        if f_c:
            hits += 1
            one.check_hit(kind, st, comb, r_c, target, mask)
    print("%s %s: %d/%d hits" % (one.kind_id(kind), name, hits, total))
    if kind in one.TWO_SIDED_KINDS and name in one.TWO_SIDED:
        assert 0.02 <= hits / total <= 0.98, (hits, total)
    if name in ("Z1", "Z6", "O1", "E") or kind == 7:
        assert hits == total


def test_onesided_ordered_windows_skip_misses():
    """Zall and Z40 are the masks with something to order: a window behind
    one of the first hits begins on a miss, so the lowest hit is not the
    window's first rank."""
    for kind in one.TWO_SIDED_KINDS:
        for name in one.TWO_SIDED:
            hits = one.hit_ranks(kind, name)
            windows = one.ordered_windows(kind, name)
            assert len(windows) == one.FIRST_HITS + 1
            assert any(begin not in hits for begin, _ in windows), (kind, name)


def test_found3_onesided_is_found3_on_two_sided_masks():
    """The rule extends found3: on the sparse masks of the per-rank cases
    the two agree on every rank."""
    case = (3, 24, 6)
    st, target, mask, _ = orc.case_setup(case)
    tabs = [orc.tt_int(st.gate(i)["table"]) for i in range(case[1])]
    t, m = orc.tt_int(target), orc.tt_int(mask)
    for comb, verdict, _, _ in orc.case_reference(case):
        g = [tabs[i] for i in comb]
        assert orc.found3_onesided(g, t, m) == verdict == orc.found3(g, t, m)


def test_scan5_verdict_on_zall_depends_on_the_seed():
    """Why the CPU scan with the same seed, and no existence oracle, is the
    reference on these masks: lut_solve_layers gives up on a split whose
    random colouring forces fi to 0, so the verdict of some ranks changes
    with the seed."""
    st, target, masks, total = one.setup(5)
    eng = orc.cpu_engine(3)
    found = {seed: [bool(eng.scan_pool(5, st, target, masks["Zall"], r, r + 1,
                                       seed=seed)[0]) for r in range(total)]
             for seed in (7, 8)}
    assert found[7] == [row[1] for row in one.reference(5, "Zall")]
    differ = sum(a != b for a, b in zip(found[7], found[8]))
    print("k=5 Zall: %d ranks differ between seeds 7 and 8" % differ)
    assert differ >= 1


# --- large pools ------------------------------------------------------------

@pytest.mark.parametrize("case", lg.ORDERED_CASES, ids=lg.case_id)
def test_large_pool_windows_hold_a_second_hit(case):
    """The ordered-sentinel windows test the election only where a window
    holds more than one hit: at least a third per (kind, pool). Every CPU
    hit validates and lies at or below its sentinel."""
    kind, n = case
    st, _ = sen.pool(n)
    ref = lg.ordered_reference(case)
    for (comb, r, target, begin, end), (f_c, r_c, _) in zip(
            lg.ordered_windows(case), ref):
        assert f_c and begin <= r < end
        lg.assert_hit_valid(kind, st, r_c, target)
    multi, count = lg.multi_hit_windows(case)
    print("%s: %d of %d windows hold a second hit"
          % (lg.case_id(case), multi, count))
    assert 3 * multi >= count


@pytest.mark.parametrize("case", lg.ANYWHERE_CASES, ids=lg.case_id)
def test_large_pool_rows_hit_by_their_last_rank(case):
    """With gate n - 1's table as the target, the CPU scan of [b, b + n)
    from a row's first rank hits at or before the row's last rank."""
    kind, n = case
    st, _ = sen.pool(n)
    windows = lg.anywhere_windows(case)
    assert len(windows) == 3 * lg.DRAWS
    at_end = 0
    for (b, row_end, end), (f_c, r_c, ev_c, rank, _) in zip(
            windows, lg.anywhere_reference(case)):
        assert f_c and b <= rank <= row_end < end, (b, rank, row_end)
        assert ev_c == rank - b + 1
        assert end - b <= n
        lg.assert_hit_valid(kind, st, r_c, lg.anywhere_target(n))
        at_end += rank == row_end
    print("%s: %d of %d hits on the row's last rank"
          % (lg.case_id(case), at_end, len(windows)))


def test_large_pool_sentinel_lists():
    for n in (200, 500):
        total = math.comb(n, 7)
        ranks = [orc.rank(c, n) for c in lg.sept_sentinels(n)]
        assert total - 1 in ranks
        assert total - math.comb(n - 1, 7) in ranks   # the first with a = 1
    for n in (130, 450, 500):
        combs = lg.shared_sentinels(n)
        ranks = [orc.rank(c, n) for c in combs]
        assert 0 in ranks and math.comb(n, 4) - 1 in ranks
        for c in combs:
            assert list(c) == sorted(set(c)) and 0 <= c[0] and c[3] < n
        # First, a middle and last d of a row.
        assert {(0, 1, 2, 3), (0, 1, 2, n - 1)} <= set(combs)
        assert any(c[:3] == (0, 1, 2) and 3 < c[3] < n - 1 for c in combs)


def test_window_case_has_unsolvable_runs():
    """The k=7 window test on the GPU derives its windows from these."""
    runs = orc.unsolvable_runs7(orc.WINDOW7_CASE)
    assert len(runs) >= 10
    ref = orc.case_reference(orc.WINDOW7_CASE)
    eng = orc.cpu_engine(7)
    st, target, mask, total = orc.case_setup(orc.WINDOW7_CASE)
    for begin, end, feasible in runs:
        assert feasible >= 1
        assert not any(ref[r][1].solvable for r in range(begin, end))
        assert end == total or ref[end][1].solvable
        assert begin == 0 or ref[begin - 1][1].solvable
        f_c, _, ev = eng.scan_pool(7, st, target, mask, begin, end,
                                   seed=orc.SCAN_SEED)
        assert not f_c and ev == end - begin
