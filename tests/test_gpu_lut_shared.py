"""The shared-input two-LUT scan on the gfx950 kernel (k_scan4s): per-rank
verdicts against the independent oracle and against cpu_scan4s, windows on a
70-gate pool that cross the kernel's prefix batches and the id < 64 edge of
the exclusion mask, and the searches that use the scan, all under
gpu="force".
"""

import math

import pytest

import _oracle as orc
import _oracle_shared as osh
from sboxgates_amd import _core, models
from sboxgates_amd.ops import gen_lut_ttable, make_engine, scan_shared
from sboxgates_amd.utils import validate_circuit

pytestmark = pytest.mark.gpu

POOL = 70
TOTAL = math.comb(POOL, 4)
PLANT = (3, 65, 66, 69)   # shape r=3, si=0: triple (3, 65, 66), d=69, s=3


@pytest.fixture(scope="module")
def engines():
    if not _core.gpu_available():
        pytest.skip("no GPU")
    gpu, cpu = orc.make_pair(True)
    assert gpu.gpu_active
    return gpu, cpu


# --- 6. per rank -------------------------------------------------------------

@pytest.mark.parametrize("case", osh.SHARED_CASES, ids=osh.case_id)
def test_scan4s_per_rank(engines, case):
    gpu, _ = engines
    st, target, mask, total = osh.case_setup(case)
    ref = osh.case_reference(case)
    before = gpu.stats()["gpu_scans"]
    for r, (comb, verdict, _, f_c, r_c) in enumerate(ref):
        f_g, r_g, ev_g = scan_shared(gpu, st, target, mask, r, r + 1,
                                     seed=orc.SCAN_SEED)
        where = (osh.case_id(case), r, comb)
        assert ev_g == 1, where
        assert f_g == verdict, where
        assert f_g == f_c, where
        # No election in a single-candidate window: the CPU's words.
        assert tuple(r_g) == r_c, (where, list(r_g), list(r_c))
    assert gpu.stats()["gpu_scans"] == before + total


# --- 7. windows on a 70-gate pool --------------------------------------------

@pytest.fixture(scope="module")
def pool70(engines):
    _, cpu = engines
    st = cpu.initial_state()
    st.grow_pool_random(POOL, orc.POOL_SEED + POOL)
    assert st.num_gates == POOL
    return st


def mid_row_window():
    """A window that begins and ends in the middle of a row; it holds
    combinations with excluded gates (2 and 5 lead some) and tail gates on
    both sides of id 64."""
    begin = orc.checked_rank([1, 4, 30, 45], POOL)
    end = orc.checked_rank([6, 20, 60, 65], POOL)
    assert 0 < begin < end < TOTAL
    return begin, end


@pytest.mark.parametrize("excl", [0, osh.EXCL], ids=["all", "excl"])
def test_scan4s_counts(engines, pool70, excl):
    gpu, cpu = engines
    target = cpu.target(0)
    full = _core.mask_for_inputs(8)
    sparse = orc.sparse_mask(7070, 10, target)
    for mask, (begin, end) in ((full, (0, TOTAL)), (sparse, mid_row_window())):
        want = scan_shared(cpu, pool70, target, mask, begin, end,
                           count_all=True, excl=excl)
        got = scan_shared(gpu, pool70, target, mask, begin, end,
                          count_all=True, excl=excl)
        assert not got[0] and not want[0]
        assert got[2] == want[2], (begin, end, excl)
        if excl == 0:
            assert got[2] == end - begin
        else:
            assert 0 < got[2] < end - begin


def planted_target(st):
    def tab(i):
        return st.gate(i)["table"]
    a, b, c, d = PLANT
    t_o = gen_lut_ttable(osh.PLANT_FO, tab(a), tab(b), tab(c))
    return gen_lut_ttable(osh.PLANT_FI, t_o, tab(d), tab(a))


@pytest.mark.parametrize("excl", [0, osh.EXCL], ids=["all", "excl"])
def test_scan4s_planted(engines, pool70, excl):
    gpu, cpu = engines
    target = planted_target(pool70)
    full = _core.mask_for_inputs(8)
    orc.assert_mask_has_target1(target, full)
    r = orc.checked_rank(list(PLANT), POOL)
    want = scan_shared(cpu, pool70, target, full, r, r + 1, seed=orc.SCAN_SEED,
                       excl=excl)
    got = scan_shared(gpu, pool70, target, full, r, r + 1, seed=orc.SCAN_SEED,
                      excl=excl)
    assert want[0] and got[0]
    assert (tuple(got[1]), got[2]) == (tuple(want[1]), 1)
    osh.assert_hit_layout(got[1], PLANT)
    orc.assert_hit_valid(5, pool70, got[1], target, full)
    # Whole range: any valid hit inside it.
    found, res, ev = scan_shared(gpu, pool70, target, full, 0, TOTAL,
                                 seed=orc.SCAN_SEED, excl=excl)
    assert found and 0 < ev <= TOTAL
    comb = sorted(set(res[2:7]))
    assert len(comb) == 4 and comb[-1] < POOL
    osh.assert_hit_layout(res, comb)
    orc.assert_hit_valid(5, pool70, res, target, full)
    assert not any(g < 64 and (excl >> g) & 1 for g in comb)


def test_scan4s_dense_miss(engines, pool70):
    gpu, cpu = engines
    target = cpu.target(0)
    full = _core.mask_for_inputs(8)
    begin, end = mid_row_window()
    end = begin + 200_000
    for excl in (0, osh.EXCL):
        want = scan_shared(cpu, pool70, target, full, begin, end,
                           seed=orc.SCAN_SEED, excl=excl)
        assert not want[0]
        got = scan_shared(gpu, pool70, target, full, begin, end,
                          seed=orc.SCAN_SEED, excl=excl)
        assert not got[0] and got[2] == want[2]


# --- 8. planted search on the GPU --------------------------------------------

@pytest.mark.parametrize("num_inputs", [4, 6])
def test_planted_search_gpu(engines, num_inputs):
    for seed in (1, 2, 3):
        luts, stats = osh.planted_search(num_inputs, seed, gpu="force",
                                         lut_shared=True)
        assert luts == 2 and stats["shared_hits"] == 1, (seed, luts, stats)
        # The 3-LUT scan and the shared scan, both on the kernels.
        assert stats["gpu_scans"] >= 2 and stats["cpu_scans"] == 0, stats
        assert stats["candidates4s"] > 0


# --- 9. end to end -----------------------------------------------------------

@pytest.mark.parametrize("gpu", ["force", "off"])
def test_des_s1_shared_end_to_end(engines, gpu):
    sbox, n = models.load("des_s1")
    eng = make_engine(lut_graph=True, seed=1, gpu=gpu, lut_shared=True)
    eng.set_sbox(sbox, n)
    st = eng.initial_state()
    out = eng.create_circuit(st, eng.target(0), _core.mask_for_inputs(n))
    assert out >= 0
    st.set_output(0, out)
    assert validate_circuit(st, sbox, n, bit=0)
    stats = eng.stats()
    assert stats["candidates4s"] > 0
    if gpu == "force":
        assert stats["cpu_scans"] == 0 and stats["gpu_scans"] > 0
