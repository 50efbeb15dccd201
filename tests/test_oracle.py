"""The independent oracle of tests/_oracle.py against the CPU scans, on
single-rank windows [r, r+1) for every rank of the per-rank cases that
tests/test_gpu_per_rank.py runs on the GPU. Runs without a GPU, so the
oracle is kept honest in the suite that runs everywhere."""

import math
import random

import pytest

import _oracle as orc


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


@pytest.mark.parametrize("case", orc.PER_RANK_CASES, ids=orc.case_id)
def test_oracle_matches_cpu_scan_per_rank(case):
    k, pool, size = case
    st, target, mask, total = orc.case_setup(case)
    orc.assert_mask_has_target1(target, mask)
    threes = orc.threes_default() if k == 4 else None
    hits = 0
    for r, (comb, verdict, f_c, r_c) in enumerate(orc.case_reference(case)):
        if k == 7:
            assert not f_c or verdict, (r, comb)      # found => feasible
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
    # A case must not pass vacuously. For k=3/4/5 the oracle's verdicts equal
    # the CPU's (asserted above), so this is the share under the oracle.
    share = hits / total
    print(f"{orc.case_id(case)}: {hits}/{total} hits ({100 * share:.1f}%)")
    assert 0.02 <= share <= 0.98, share
