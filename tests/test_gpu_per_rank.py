"""Per-rank verdicts of every GPU scan against the independent oracle of
tests/_oracle.py and against the CPU scans: single-rank windows [r, r+1)
over the whole combination space of small pools, under sparse masks.

A single-candidate window leaves no winner election, so for k=3, k=4 (both
the persistent service and the one-shot kernel) and k=5 the result words
must be identical to the CPU's. For k=7 the assign kernel's winner among
orderings is a race, so only the verdict, the ids and the validity of the
hit are compared.

On the kernels before k_scan3 took its random word as cpu_scan3 does, the
k=3 result comparison failed first at case k3-pool24-mask4, rank 1, gates
(0, 1, 3): function byte 0x51 from the kernel, 0x60 from cpu_scan3.
"""

import pytest

import _oracle as orc
from sboxgates_amd import _core

pytestmark = pytest.mark.gpu

CASES = {k: [c for c in orc.PER_RANK_CASES if c[0] == k] for k in (3, 4, 5, 7)}


@pytest.fixture(scope="module")
def lut_gpu():
    if not _core.gpu_available():
        pytest.skip("no GPU")
    gpu, _ = orc.make_pair(True)
    assert gpu.gpu_active
    return gpu


def check_case(gpu, case, compare_res):
    """Scans every rank of the case on `gpu`; returns the number of scans."""
    k = case[0]
    st, target, mask, total = orc.case_setup(case)
    orc.assert_mask_has_target1(target, mask)
    threes = orc.threes_default() if k == 4 else None
    ref = orc.case_reference(case)
    assert len(ref) == total
    for r, (comb, verdict, f_c, r_c) in enumerate(ref):
        f_g, r_g, ev_g = gpu.scan_pool(k, st, target, mask, r, r + 1,
                                       seed=orc.SCAN_SEED)
        where = (orc.case_id(case), r, comb)
        assert ev_g == 1, where
        assert f_g == f_c, where
        if k == 7:
            assert not f_g or verdict, where       # found => feasible
        elif k == 4:
            assert f_g == (verdict is not None), where
        else:
            assert f_g == verdict, where
        if not f_g:
            continue
        assert orc.hit_ids(k, r_g) == comb, (where, r_g)
        orc.assert_hit_valid(k, st, r_g, target, mask, threes)
        if k == 4:
            assert (r_g[0], r_g[1]) == verdict, (where, r_g)
        if compare_res:
            assert tuple(r_g) == r_c, (where, list(r_g), list(r_c))
    return total


@pytest.mark.parametrize("case", CASES[3], ids=orc.case_id)
def test_scan3_per_rank(lut_gpu, case):
    check_case(lut_gpu, case, compare_res=True)


@pytest.mark.parametrize("case", CASES[5], ids=orc.case_id)
def test_scan5_per_rank(lut_gpu, case):
    check_case(lut_gpu, case, compare_res=True)


@pytest.mark.parametrize("case", CASES[7], ids=orc.case_id)
def test_scan7_per_rank(lut_gpu, case):
    check_case(lut_gpu, case, compare_res=False)


def fresh_k4_gpu():
    if not _core.gpu_available():
        pytest.skip("no GPU")
    gpu, _ = orc.make_pair(False, try_nots=True)
    assert gpu.gpu_active
    return gpu


@pytest.mark.parametrize("case", CASES[4], ids=orc.case_id)
def test_scan4_service_per_rank(monkeypatch, capfd, case):
    # The engine decides between service and one-shot kernel on its first
    # k=4 scan, from the environment as it is then.
    monkeypatch.delenv("SBOXGATES_NO_SVC", raising=False)
    gpu = fresh_k4_gpu()
    scans = check_case(gpu, case, compare_res=True)
    assert gpu.stats()["gpu_scans"] == scans
    # A service that fails hands its engine to the one-shot kernel and says
    # so; that must not be how this test passed.
    assert "scan service disabled" not in capfd.readouterr().err


@pytest.mark.parametrize("case", CASES[4], ids=orc.case_id)
def test_scan4_oneshot_per_rank(monkeypatch, case):
    """The same shape on the one-shot k_scan4 kernel: with SBOXGATES_NO_SVC
    set before its first k=4 scan, a fresh engine never acquires the
    service."""
    monkeypatch.setenv("SBOXGATES_NO_SVC", "1")
    gpu = fresh_k4_gpu()
    scans = check_case(gpu, case, compare_res=True)
    # Every scan of the case went through this engine's GPU path.
    stats = gpu.stats()
    assert stats["gpu_scans"] == scans and stats["cpu_scans"] == 0
