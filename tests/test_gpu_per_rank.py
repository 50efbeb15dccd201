"""Per-rank verdicts of every GPU scan against the independent oracle of
tests/_oracle.py and against the CPU scans: single-rank windows [r, r+1)
over the whole combination space of small pools, under sparse masks.

A single-candidate window leaves no winner election, so for k=3, k=4 (both
the persistent service and the one-shot kernel) and k=5 the result words
must be identical to the CPU's. For k=7 the assign kernel's winner among
orderings is a race, so only the verdict, the ids and the validity of the
hit are compared; the verdict is held to the oracle's full decomposition
verdict (found7), not only to the CPU's, with which the kernel shares its
solver.

The k=7 window tests at the end take their windows from the same per-rank
table: runs of unsolvable ranks, the same runs with the solvable rank that
ends them, the whole space, and a deep hit list of 972 feasible candidates
none of which is solvable, under the default hit buffer and under one of 64
entries that the scan has to split its range for.

On the kernels before k_scan3 took its random word as cpu_scan3 does, the
k=3 result comparison failed first at case k3-pool24-mask4, rank 1, gates
(0, 1, 3): function byte 0x51 from the kernel, 0x60 from cpu_scan3.
"""

import json
import os
import subprocess
import sys

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
            assert f_g == verdict.solvable, where
            assert verdict.feasible or not f_g, where  # found => feasible
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


# --- k=7 windows ------------------------------------------------------------

def window_case_scans():
    """(begin, end, kind) of the window scans on WINDOW7_CASE."""
    total = orc.case_setup(orc.WINDOW7_CASE)[3]
    scans = []
    for begin, end, _ in orc.unsolvable_runs7(orc.WINDOW7_CASE):
        scans.append((begin, end, "run"))
        if end < total:
            scans.append((begin, end + 1, "run+1"))
    scans.append((0, total, "whole"))
    return scans


def check_window_case(scans, results):
    """results[i] = (found, res, evaluated) of scans[i]; returns the number
    of not-found scans whose window held a feasible rank."""
    st, target, mask, total = orc.case_setup(orc.WINDOW7_CASE)
    ref = orc.case_reference(orc.WINDOW7_CASE)
    misses = 0
    for (begin, end, kind), (found, res, ev) in zip(scans, results):
        where = (begin, end, kind)
        if kind == "run":
            assert not found, where
            assert ev == end - begin, where
            assert any(ref[r][1].feasible for r in range(begin, end)), where
            misses += 1
            continue
        assert found, where
        assert ev <= end - begin, where
        orc.assert_hit_valid(7, st, res, target, mask)
        r = orc.checked_rank(orc.hit_ids(7, res), orc.WINDOW7_CASE[1])
        assert begin <= r < end and ref[r][1].solvable, (where, r)
        if kind == "run+1":
            assert r == end - 1, (where, r)
            assert orc.hit_ids(7, res) == ref[end - 1][0], where
    return misses


def check_deep(results):
    """results = (found, res, evaluated) of the two DEEP7_WINDOWS."""
    st, target, mask = orc.deep7_setup()
    (found0, _, ev0), (found1, res1, ev1) = results
    assert not found0
    assert ev0 == orc.DEEP7_FIRST
    assert found1
    assert orc.hit_ids(7, res1) == orc.DEEP7_COMB
    orc.assert_hit_valid(7, st, res1, target, mask)
    assert ev1 <= orc.DEEP7_FIRST + 1


def test_scan7_windows_from_oracle_table(lut_gpu):
    st, target, mask, _ = orc.case_setup(orc.WINDOW7_CASE)
    scans = window_case_scans()
    results = [lut_gpu.scan_pool(7, st, target, mask, begin, end,
                                 seed=orc.SCAN_SEED)
               for begin, end, _ in scans]
    assert check_window_case(scans, results) >= 10


def test_scan7_deep_unsolvable_hit_list(lut_gpu):
    """972 filter hits, none solvable, then one more window that ends on the
    first solvable rank (tests/test_oracle.py re-derives both facts on the
    host): k_scan7_assign over a hit list that is all misses."""
    st, target, mask = orc.deep7_setup()
    check_deep([lut_gpu.scan_pool(7, st, target, mask, begin, end,
                                  seed=orc.SCAN_SEED)
                for begin, end in orc.DEEP7_WINDOWS])


@pytest.fixture(scope="module")
def cap64_results(lut_gpu):
    """The deep windows and the window-case scans again, in a fresh process
    whose hit buffer holds 64 entries."""
    scans = window_case_scans()
    args = ["deep:%d:%d" % w for w in orc.DEEP7_WINDOWS]
    args += ["case:%d:%d" % (begin, end) for begin, end, _ in scans]
    env = dict(os.environ)
    env["SBOXGATES_HIT_CAP"] = "64"
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                          "_scan7_worker.py")
    # The child starts an interpreter and an engine and runs some 30 scans,
    # the two deep ones in a few dozen kernel launches each: seconds.
    r = subprocess.run([sys.executable, worker] + args, env=env,
                       capture_output=True, text=True, timeout=90)
    assert r.returncode == 0, r.stderr
    results = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(results) == len(args)
    return scans, results


def test_scan7_deep_hit_list_split_by_small_cap(cap64_results):
    """972 hits against a buffer of 64 force repeated halving of the range.
    The not-found window must still count every rank exactly once (the
    accounting invariant in GpuEngine::scan), and the found window must
    still end on rank DEEP7_FIRST."""
    _, results = cap64_results
    check_deep(results[:2])


def test_scan7_windows_small_cap(cap64_results):
    scans, results = cap64_results
    assert check_window_case(scans, results[2:]) >= 10
