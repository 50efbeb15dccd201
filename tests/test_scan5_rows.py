"""k_scan5 row-segment walk (gfx950) against cpu_scan5.

The 5-LUT kernel walks each triple's (d, e) pairs as row segments: the d
side is hoisted once per segment, a screen on one live cell runs over the
e side, and only what passes reaches the other cells and the solver. These
tests pin the parts that can go wrong there: window clipping at every
boundary, the flat rank handed to the solver, the all-survivor case of
empty live masks, the per-row exclusion arithmetic and long rows cut into
several segments.

Same two engines as tests/test_gpu.py (rijndael, gpu="force" vs gpu="off");
cpu_scan5 is the reference throughout.
"""

import random
import struct

import pytest

from sboxgates_amd import _core, models
from sboxgates_amd.ops import (combination_rank, gen_lut_ttable, make_engine,
                               mask_for_inputs, n_choose_k, nth_combination,
                               tt_eq_mask)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engines():
    if not _core.gpu_available():
        pytest.skip("no GPU")
    gpu = make_engine(lut_graph=True, seed=1, gpu="force", save_states=False)
    cpu = make_engine(lut_graph=True, seed=1, gpu="off", save_states=False)
    sbox, n = models.load("rijndael")
    gpu.set_sbox(sbox, n)
    cpu.set_sbox(sbox, n)
    assert gpu.gpu_active
    return gpu, cpu


def make_pool(engine, pool, seed):
    st = engine.initial_state()
    if pool > st.num_gates:
        st.grow_pool_random(pool, seed)
    assert st.num_gates == pool
    return st


def plant(st, ids, rng):
    """A 5-LUT-decomposable target over the gates `ids`, composed as in
    test_gpu.test_planted_solutions_found_and_valid."""
    tabs = [st.gate(i)["table"] for i in ids]
    t_o = gen_lut_ttable(rng.randrange(256), tabs[0], tabs[1], tabs[2])
    return gen_lut_ttable(rng.randrange(256), t_o, tabs[3], tabs[4])


def realizes(st, res, target, mask):
    t_o = gen_lut_ttable(res[0], st.gate(res[2])["table"],
                         st.gate(res[3])["table"], st.gate(res[4])["table"])
    got = gen_lut_ttable(res[1], t_o, st.gate(res[5])["table"],
                         st.gate(res[6])["table"])
    return tt_eq_mask(target, got, mask)


def sparse_mask(positions):
    words = [0, 0, 0, 0]
    for i in positions:
        words[i // 64] |= 1 << (i % 64)
    return struct.pack("<4Q", *words)


def target_bit(target, i):
    return (target[i // 8] >> (i % 8)) & 1


# ---------------------------------------------------------------------------
# 1. Every window at n = 8.
# ---------------------------------------------------------------------------
def test_every_window_n8(engines):
    """C(8,5) = 56 combinations, triples with m = 2..5 (single-pair row,
    odd and even row counts, the last row): all 1596 windows count right."""
    gpu, cpu = engines
    st = make_pool(gpu, 8, 0)
    target = gpu.target(0)
    mask = mask_for_inputs(8)
    total = n_choose_k(8, 5)
    assert total == 56
    windows = 0
    for b in range(total):
        for e in range(b + 1, total + 1):
            _, _, ev_g = gpu.scan_pool(5, st, target, mask, b, e, seed=2,
                                       count_all=True)
            _, _, ev_c = cpu.scan_pool(5, st, target, mask, b, e, seed=2,
                                       count_all=True)
            assert ev_g == e - b, (b, e, ev_g)
            assert ev_g == ev_c, (b, e, ev_g, ev_c)
            windows += 1
    assert windows == 1596


# ---------------------------------------------------------------------------
# 2. Per-rank verdicts at n = 9 and n = 10.
# ---------------------------------------------------------------------------
def planted_combinations(n):
    m = n - 3  # pairs of the triple (0, 1, 2) run over m gates
    mid = 3 + (m - 2) // 2  # the middle one of its m - 1 rows
    return {
        "first": [0, 1, 2, 3, 4],
        "last": [n - 5, n - 4, n - 3, n - 2, n - 1],
        "row_end": [0, 1, 2, 3, n - 1],  # d = c + 1, e = n - 1
        "middle_row": [0, 1, 2, mid, mid + 1],
    }


@pytest.mark.parametrize("which", ["first", "last", "row_end", "middle_row"])
@pytest.mark.parametrize("n", [9, 10])
def test_per_rank_verdicts(engines, n, which):
    """Single-candidate windows [r, r+1) for every rank r: same verdict on
    both engines, the planted rank found on both, every GPU hit valid, and
    res equal to the CPU's (one candidate, solver seeded by its flat rank).
    """
    gpu, cpu = engines
    st = make_pool(gpu, n, 0xC0 + n)
    mask = mask_for_inputs(8)
    ids = planted_combinations(n)[which]
    target = plant(st, ids, random.Random(1000 * n + sum(ids)))
    planted_rank = combination_rank(ids, n)
    total = n_choose_k(n, 5)
    assert 0 <= planted_rank < total
    res_mismatch = []
    for r in range(total):
        f_g, r_g, _ = gpu.scan_pool(5, st, target, mask, r, r + 1, seed=7)
        f_c, r_c, _ = cpu.scan_pool(5, st, target, mask, r, r + 1, seed=7)
        assert f_g == f_c, (r, f_g, f_c)
        if r == planted_rank:
            assert f_g and f_c, "planted rank not found"
        if f_g:
            assert sorted(r_g[2:7]) == list(nth_combination(r, n, 5)), r
            assert realizes(st, r_g, target, mask), r
            if list(r_g) != list(r_c):
                res_mismatch.append((r, list(r_g), list(r_c)))
    print("res mismatches:", res_mismatch)
    assert not res_mismatch


# ---------------------------------------------------------------------------
# 3. Sparse masks at n = 12.
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["random1", "random2", "random6", "random16",
                                  "ones_only6"])
def test_sparse_masks_n12(engines, case):
    """Masks of 1, 2, 6 and 16 positions, one of them inside the target's
    ones (no live cell in any triple: every pair goes to the exact test)."""
    gpu, cpu = engines
    n = 12
    st = make_pool(gpu, n, 0x12C)
    target = gpu.target(0)
    rng = random.Random(sum(map(ord, case)))
    if case == "ones_only6":
        ones = [i for i in range(256) if target_bit(target, i)]
        positions = rng.sample(ones, 6)
        assert all(target_bit(target, i) for i in positions)
    else:
        positions = rng.sample(range(256), int(case[len("random"):]))
    mask = sparse_mask(positions)
    total = n_choose_k(n, 5)

    _, _, ev_g = gpu.scan_pool(5, st, target, mask, 0, total, seed=4,
                               count_all=True)
    _, _, ev_c = cpu.scan_pool(5, st, target, mask, 0, total, seed=4,
                               count_all=True)
    assert ev_g == ev_c == total

    f_g, r_g, _ = gpu.scan_pool(5, st, target, mask, 0, total, seed=4)
    f_c, _, _ = cpu.scan_pool(5, st, target, mask, 0, total, seed=4)
    assert f_g == f_c
    if f_g:
        assert realizes(st, r_g, target, mask)

    hits = 0
    for r in rng.sample(range(total), 60):
        f_g, r_g, _ = gpu.scan_pool(5, st, target, mask, r, r + 1, seed=4)
        f_c, _, _ = cpu.scan_pool(5, st, target, mask, r, r + 1, seed=4)
        assert f_g == f_c, (r, f_g, f_c)
        if f_g:
            hits += 1
            assert sorted(r_g[2:7]) == list(nth_combination(r, n, 5)), r
            assert realizes(st, r_g, target, mask), r
    print(case, "hits in 60 ranks:", hits)


# ---------------------------------------------------------------------------
# 4. Exclusion at n = 70 (gate ids >= 64 exist).
# ---------------------------------------------------------------------------
def excl_masks():
    rng = random.Random(0xE8C1)
    rnd8 = 0
    for b in rng.sample(range(64), 8):
        rnd8 |= 1 << b
    return {"gate0": 1 << 0, "gate63": 1 << 63, "gate31": 1 << 31,
            "random8": rnd8}


@pytest.mark.parametrize("which", ["gate0", "gate63", "gate31", "random8"])
def test_exclusion_counts_n70(engines, which):
    """evaluated under an exclusion mask is the number of combinations in
    the window without an excluded gate — not e - b — and must equal the
    CPU's; verdicts agree."""
    gpu, cpu = engines
    n = 70
    st = make_pool(gpu, n, 0x70)
    target = gpu.target(0)
    mask = mask_for_inputs(8)
    excl = excl_masks()[which]
    total = n_choose_k(n, 5)
    rng = random.Random(excl & 0xFFFFFFFF)
    windows = [(0, 2_000_000)]
    for length in (1, 77, 4_000, 60_000, 250_000, 700_000):
        b = rng.randrange(total - length)
        windows.append((b, b + length))
    assert all(e - b <= 2_000_000 for b, e in windows)
    for b, e in windows:
        _, _, ev_g = gpu.scan_pool(5, st, target, mask, b, e, seed=6,
                                   count_all=True, excl=excl)
        _, _, ev_c = cpu.scan_pool(5, st, target, mask, b, e, seed=6,
                                   count_all=True, excl=excl)
        assert ev_g == ev_c, (which, b, e, ev_g, ev_c)
        f_g, r_g, _ = gpu.scan_pool(5, st, target, mask, b, e, seed=6,
                                    excl=excl)
        f_c, _, _ = cpu.scan_pool(5, st, target, mask, b, e, seed=6,
                                  excl=excl)
        assert f_g == f_c, (which, b, e)
        if f_g:
            assert realizes(st, r_g, target, mask)
            assert not any(g < 64 and (excl >> g) & 1 for g in r_g[2:7])
    # The first window starts inside a = 0; with gate 0 excluded it must
    # count far less than its length.
    if which == "gate0":
        _, _, ev = gpu.scan_pool(5, st, target, mask, 0, 2_000_000, seed=6,
                                 count_all=True, excl=excl)
        assert ev == 2_000_000 - n_choose_k(n - 1, 4)


def test_exclusion_planted_n70(engines):
    """A planted combination holding an excluded gate is never reported;
    one holding none is found."""
    gpu, cpu = engines
    n = 70
    st = make_pool(gpu, n, 0x70)
    mask = mask_for_inputs(8)
    rng = random.Random(0x91A)
    excl = (1 << 5) | (1 << 40) | (1 << 63)
    for ids, expect in (([2, 9, 17, 40, 66], False),   # d excluded
                        ([2, 9, 17, 41, 63], False),   # e excluded
                        ([5, 9, 17, 41, 66], False),   # prefix excluded
                        ([2, 9, 17, 41, 66], True)):
        target = plant(st, ids, rng)
        rank = combination_rank(ids, n)
        for b, e in ((rank, rank + 1), (rank - 1500, rank + 1500)):
            f_g, r_g, _ = gpu.scan_pool(5, st, target, mask, b, e, seed=8,
                                        excl=excl)
            f_c, _, _ = cpu.scan_pool(5, st, target, mask, b, e, seed=8,
                                      excl=excl)
            assert f_g == f_c, (ids, b, e)
            if expect:
                assert f_g, ids
            if e == b + 1:
                assert f_g == expect, ids
            if f_g:
                assert realizes(st, r_g, target, mask)
                assert not any(g < 64 and (excl >> g) & 1 for g in r_g[2:7])
        # Without the exclusion the same combination is a hit.
        f_g, _, _ = gpu.scan_pool(5, st, target, mask, rank, rank + 1, seed=8)
        assert f_g, ids


# ---------------------------------------------------------------------------
# 5. Long rows at n = 90, full mask.
# ---------------------------------------------------------------------------
def long_row_windows():
    n = 90
    span = 3_000_000
    mid_row_start = combination_rank([0, 1, 2, 10, 50], n)
    mid_row_end = combination_rank([3, 8, 20, 30, 61], n) + 1
    a_change = n_choose_k(n - 1, 4)  # first rank with a = 1
    return {
        "starts_mid_row": (mid_row_start, mid_row_start + span),
        "ends_mid_row": (mid_row_end - span, mid_row_end),
        "straddles_a": (a_change - span // 2, a_change + span // 2),
    }


@pytest.mark.parametrize("which", ["starts_mid_row", "ends_mid_row",
                                   "straddles_a"])
def test_long_rows_n90(engines, which):
    gpu, cpu = engines
    n = 90
    st = make_pool(gpu, n, 0x90)
    target = gpu.target(0)
    mask = mask_for_inputs(8)
    b, e = long_row_windows()[which]
    assert 0 <= b < e <= n_choose_k(n, 5) and e - b == 3_000_000
    _, _, ev_g = gpu.scan_pool(5, st, target, mask, b, e, seed=9,
                               count_all=True)
    _, _, ev_c = cpu.scan_pool(5, st, target, mask, b, e, seed=9,
                               count_all=True)
    assert ev_g == ev_c == e - b
    f_g, r_g, _ = gpu.scan_pool(5, st, target, mask, b, e, seed=9)
    f_c, _, _ = cpu.scan_pool(5, st, target, mask, b, e, seed=9)
    assert f_g == f_c
    if f_g:
        assert realizes(st, r_g, target, mask)


def test_long_row_planted_at_row_end_n90(engines):
    """A hit at e = n - 1 of the longest row (86 pairs: several segments),
    found through a 64-rank window around it."""
    gpu, cpu = engines
    n = 90
    st = make_pool(gpu, n, 0x90)
    mask = mask_for_inputs(8)
    ids = [0, 1, 2, 3, n - 1]
    target = plant(st, ids, random.Random(0x5EED))
    rank = combination_rank(ids, n)
    b, e = rank - 32, rank + 32
    assert b >= 0
    f_g, r_g, _ = gpu.scan_pool(5, st, target, mask, b, e, seed=10)
    f_c, _, _ = cpu.scan_pool(5, st, target, mask, b, e, seed=10)
    assert f_c and f_g
    assert realizes(st, r_g, target, mask)
    f_g, r_g, _ = gpu.scan_pool(5, st, target, mask, rank, rank + 1, seed=10)
    assert f_g
    assert sorted(r_g[2:7]) == ids
