"""GPU scans at the pool sizes a long search reaches: the 7-LUT kernels at
pools 200 and 500 (MAX_GATES), the shared-input scan at 130, 450 and 500,
and the ordered scans of every kind at those sizes. There the closed-form
binomials cf4 to cf7, first_of_rank, the prefix-window decoders, the host's
quad slicing, dev_rank7, the packed `best` words and ordered_result work on
their largest arguments; a disagreement in the ordered path is no wrong word
but the exception "hits on the GPU and misses on the CPU", which ends a
search.

Fixtures and CPU references are those of tests/_oracle_large.py. Every
expectation is a CPU scan of the same window, the pure-Python rank and
unrank of _oracle.py, or the re-evaluation of the hit; none comes from a GPU
run. Windows with a second CPU hit (tests/test_oracle.py asserts at least a
third per case): k=3 pool 500 128 of 223, k=4 pool 500 112 of 223, k=5 pool
450 39 of 54, pool 500 48 of 54, pool 120 42 of 54, shared pool 450 10 of
13, pool 500 7 of 13, k=7 pools 200 and 500 11 of 11 each.
"""

import math
import random

import pytest

import _oracle as orc
import _oracle_large as lg
import _oracle_shared as osh
import test_gpu_sentinels as sen
from sboxgates_amd import _core

pytestmark = pytest.mark.gpu

FULL, SEED = lg.FULL, lg.SEED


def need_gpu():
    if not _core.gpu_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def lut_pair():
    need_gpu()
    gpu, cpu = orc.make_pair(True)
    assert gpu.gpu_active
    return gpu, cpu


@pytest.fixture(scope="module")
def lut_ordered():
    need_gpu()
    gpu = orc.rijndael_engine(True, gpu="force", ordered=True)
    assert gpu.gpu_active
    return gpu


def on_gpu(gpu, before):
    """The scans since `before` (a stats() of the engine) ran on the GPU."""
    stats = gpu.stats()
    assert stats["cpu_scans"] == 0, stats
    assert stats["gpu_scans"] > before["gpu_scans"], stats


# --- 1. k=7 sentinels at pools 200 and 500 ----------------------------------

@pytest.mark.parametrize("n", [200, 500])
def test_scan7_sentinels(lut_pair, n):
    gpu, cpu = lut_pair
    before = gpu.stats()
    combs = lg.sept_sentinels(n)
    # Both ends of cf7(n) - cf7(n - a): the last quad and the first a = 1.
    assert tuple(range(n - 7, n)) in combs and tuple(range(1, 8)) in combs
    assert orc.rank(range(1, 8), n) == math.comb(n, 7) - math.comb(n - 1, 7)
    rng = random.Random(0x7700 + n)
    for comb in combs:
        sen.check_sentinel(gpu, cpu, 7, n, comb, rng)
    on_gpu(gpu, before)


# --- 2. shared-scan sentinels at pools 130, 450 and 500 ---------------------

def check_shared_sentinel(gpu, cpu, n, comb, rng):
    """test_gpu_sentinels.check_sentinel for the shared-input scan."""
    st, tabs = sen.pool(n)
    comb = list(comb)
    assert len(comb) == 4 and comb == sorted(set(comb)) and comb[-1] < n
    total = math.comb(n, 4)
    r = orc.checked_rank(comb, n)
    assert orc.checked_unrank(r, n, 4) == comb
    target, shape = lg.plant_shared([tabs[i] for i in comb], rng)
    orc.assert_mask_has_target1(target, FULL)
    where = (n, comb, r, shape)

    f_g, r_g, _ = gpu.scan_shared(st, target, FULL, r, r + 1, seed=SEED)
    f_c, r_c, _ = cpu.scan_shared(st, target, FULL, r, r + 1, seed=SEED)
    assert f_c, where
    assert f_g, where
    for res in (r_g, r_c):
        osh.assert_hit_layout(res, tuple(comb))
    orc.assert_hit_valid(5, st, r_g, target, FULL)

    a, b = max(0, r - 2000), min(total, r + 2001)
    f_g, r_g, _ = gpu.scan_shared(st, target, FULL, a, b, seed=SEED)
    f_c, r_c, _ = cpu.scan_shared(st, target, FULL, a, b, seed=SEED)
    assert f_c, (where, a, b)
    assert f_g, (where, a, b)
    orc.assert_hit_valid(5, st, r_g, target, FULL)
    orc.assert_hit_valid(5, st, r_c, target, FULL)
    ids = lg.hit_ids("s", r_g)
    osh.assert_hit_layout(r_g, tuple(ids))
    assert a <= orc.checked_rank(ids, n) < b, (where, a, b, list(r_g))


@pytest.mark.parametrize("n", [130, 450, 500])
def test_shared_sentinels(lut_pair, n):
    gpu, cpu = lut_pair
    before = gpu.stats()
    combs = lg.shared_sentinels(n)
    assert (0, 1, 2, 3) in combs and tuple(range(n - 4, n)) in combs
    assert len(combs) >= 12
    rng = random.Random(0x4500 + n)
    for comb in combs:
        check_shared_sentinel(gpu, cpu, n, comb, rng)
    on_gpu(gpu, before)


# --- 3. windows that begin anywhere in the rank space -----------------------

def check_anywhere(gpu, gpu_ord, case):
    """The window [b, b + n) from the first rank b of a drawn prefix's row,
    target gate n - 1: the row's last rank hits.

    An unordered scan reports whichever hit wins its election, and a row is
    shorter than n ranks, so that the window reaches into the next rows,
    whose last ranks hit as well: the hit of the default engine is held to
    [b, row end] where the CPU scan finds no hit behind the row's end, and
    in every draw by a second scan of the row alone."""
    kind, n = case
    st, _ = sen.pool(n)
    target = lg.anywhere_target(n)
    ref = lg.anywhere_reference(case)
    in_row = 0
    for (b, row_end, end), (f_c, r_c, ev_c, rank_c, later) in zip(
            lg.anywhere_windows(case), ref):
        where = (lg.case_id(case), b, row_end, end)
        assert f_c and b <= rank_c <= row_end, where
        for stop in (end, row_end + 1):
            f_g, r_g, ev_g = lg.scan(gpu, kind, st, target, FULL, b, stop,
                                     seed=SEED)
            assert f_g, (where, stop)
            lg.assert_hit_valid(kind, st, r_g, target)
            rank_g = orc.rank(lg.hit_ids(kind, r_g), n)
            assert b <= rank_g < stop, (where, stop, rank_g)
            if stop == row_end + 1 or not later:
                assert b <= rank_g <= row_end, (where, stop, rank_g)
            in_row += b <= rank_g <= row_end
        f_o, r_o, ev_o = lg.scan(gpu_ord, kind, st, target, FULL, b, end,
                                 seed=SEED)
        assert f_o, where
        assert tuple(r_o) == r_c, (where, list(r_o), list(r_c))
        assert 1 <= ev_o <= n, (where, ev_o)
    return in_row


@pytest.mark.parametrize("case", lg.ANYWHERE_CASES, ids=lg.case_id)
def test_begin_anywhere(lut_pair, lut_ordered, case):
    gpu, _ = lut_pair
    before = gpu.stats(), lut_ordered.stats()
    in_row = check_anywhere(gpu, lut_ordered, case)
    print("%s: %d of %d default-mode hits inside the row"
          % (lg.case_id(case), in_row, 2 * len(lg.anywhere_windows(case))))
    on_gpu(gpu, before[0])
    on_gpu(lut_ordered, before[1])


# --- 4. ordered sentinels ---------------------------------------------------

def check_ordered_sentinels(gpu_ord, case):
    """Every window of +-2000 ranks around a sentinel: the CPU scan's res,
    word for word. Returns the number of scans."""
    kind, n = case
    st, _ = sen.pool(n)
    windows = lg.ordered_windows(case)
    ref = lg.ordered_reference(case)
    multi, count = lg.multi_hit_windows(case)
    assert 3 * multi >= count, (lg.case_id(case), multi, count)
    for (comb, r, target, begin, end), (f_c, r_c, _) in zip(windows, ref):
        where = (lg.case_id(case), comb, r, begin, end)
        f_g, r_g, ev_g = lg.scan(gpu_ord, kind, st, target, FULL, begin, end,
                                 seed=SEED)
        assert f_g and f_c, where
        assert tuple(r_g) == r_c, (where, list(r_g), list(r_c))
        assert 1 <= ev_g <= end - begin, where
        lg.assert_hit_valid(kind, st, r_g, target)
    return len(windows)


LUT_ORDERED_CASES = [c for c in lg.ORDERED_CASES if c[0] != 4]


@pytest.mark.parametrize("case", LUT_ORDERED_CASES, ids=lg.case_id)
def test_ordered_sentinels(lut_ordered, case):
    if case[0] == 5:
        # The host gives the two large pools to k_scan5_wave by itself and
        # pool 120 to the batch kernel's wide walk.
        assert (case[1] >= _core.scan5_wave_min_pool()) == (case[1] != 120)
        assert case[1] - 3 > _core.SCAN5_WIDE_MIN_ROW
    before = lut_ordered.stats()
    scans = check_ordered_sentinels(lut_ordered, case)
    on_gpu(lut_ordered, before)
    assert lut_ordered.stats()["gpu_scans"] == before["gpu_scans"] + scans


@pytest.mark.parametrize("path", ["service", "oneshot"])
def test_scan4_ordered_sentinels_pool500(monkeypatch, capfd, path):
    need_gpu()
    # The engine decides between service and one-shot kernel on its first
    # k=4 scan, from the environment as it is then.
    if path == "service":
        monkeypatch.delenv("SBOXGATES_NO_SVC", raising=False)
    else:
        monkeypatch.setenv("SBOXGATES_NO_SVC", "1")
    gpu = orc.rijndael_engine(False, gpu="force", ordered=True, try_nots=True)
    assert gpu.gpu_active
    scans = check_ordered_sentinels(gpu, (4, 500))
    stats = gpu.stats()
    assert stats["gpu_scans"] == scans and stats["cpu_scans"] == 0
    # A service that fails hands its engine to the one-shot kernel and says
    # so; that must not be how this test passed.
    assert "scan service disabled" not in capfd.readouterr().err


# --- 5. exclusion counts at pool 500 ----------------------------------------

@pytest.mark.parametrize("kind", lg.EXCL_KINDS, ids=lg.kind_id)
def test_exclusion_counts_pool500(lut_pair, kind):
    """test_gpu_sentinels.test_scan7_exclusions_pool70's scheme at MAX_GATES:
    count_all over windows of 200,000 ranks under exclusion sets."""
    gpu, cpu = lut_pair
    before = gpu.stats()
    n, w = lg.EXCL_POOL, lg.EXCL_WINDOW
    st, _ = sen.pool(n)
    target = gpu.target(0)
    total = math.comb(n, lg.width(kind))
    windows = lg.exclusion_windows(kind)
    last = lg.last_window_walk(kind)
    acted = False
    for excl in lg.exclusion_sets():
        for begin in windows:
            _, _, ev_g = lg.scan(gpu, kind, st, target, FULL, begin, begin + w,
                                 count_all=True, excl=excl)
            _, _, ev_c = lg.scan(cpu, kind, st, target, FULL, begin, begin + w,
                                 count_all=True, excl=excl)
            assert ev_g == ev_c, (kind, hex(excl), begin, ev_g, ev_c)
            acted = acted or 0 < ev_c < w
            if begin == total - w:
                assert ev_g == sum(1 for m in last if not m & excl), hex(excl)
    assert acted
    on_gpu(gpu, before)
