"""Ordered GPU scans (make_engine(ordered=True)): every scan kind returns what
the matching CPU scan returns for the same request and window, the same
`found` and a res[10] equal word for word, and a whole gpu="force" search
finds the circuit that the gpu="off" search of the same seed finds.

Every expectation comes from the CPU scans or from the per-rank tables of
_oracle.py, which tests/test_oracle.py holds to the independent oracle; none
comes from the ordered GPU path. Each scan under test runs once per window:
the windows are the coverage. A window that reaches past several hits is
where an unordered winner election shows, so the windows begin behind each
of the first hits and the tests assert that such a window holds at least
two.

`evaluated` on a miss is the window's size (what the CPU scan counts where
nothing is excluded); on a hit it is only required to lie in [1, size].
"""

import json
import math
import os
import subprocess
import sys

import pytest

import _oracle as orc
import test_ordered
import test_search_pinned as pinned
from sboxgates_amd import _core

pytestmark = pytest.mark.gpu

CASES = {k: [c for c in orc.PER_RANK_CASES if c[0] == k] for k in (3, 4, 5, 7)}
FIRST_HITS = 8


def ordered_gpu(lut_graph, **kw):
    if not _core.gpu_available():
        pytest.skip("no GPU")
    gpu = orc.rijndael_engine(lut_graph, gpu="force", ordered=True, **kw)
    assert gpu.gpu_active
    return gpu


@pytest.fixture(scope="module")
def lut_gpu():
    return ordered_gpu(True)


def hit_windows(hits, total):
    """(begin, end, must_hit) windows around the first hits h_0 < h_1 < ...:
    the whole space, from behind each hit to the end, from behind each hit
    to just before the next (a miss) and to the next inclusive."""
    windows = [(0, total, True)]
    for i in range(min(FIRST_HITS, len(hits) - 1)):
        h, nxt = hits[i], hits[i + 1]
        windows.append((h + 1, total, True))
        if h + 1 < nxt:
            windows.append((h + 1, nxt, False))
        windows.append((h + 1, nxt + 1, True))
    return windows


# --- 1. windows over the per-rank tables --------------------------------------

def check_case_windows(gpu, case):
    """Returns the number of scans."""
    k = case[0]
    st, target, mask, total = orc.case_setup(case)
    ref = orc.case_reference(case)
    hits = [r for r, row in enumerate(ref) if row[2]]
    # Every window that runs to `total` holds at least two hits.
    assert len(hits) >= FIRST_HITS + 2, (orc.case_id(case), len(hits))
    windows = hit_windows(hits, total)
    for begin, end, must_hit in windows:
        where = (orc.case_id(case), begin, end)
        inside = [h for h in hits if begin <= h < end]
        assert bool(inside) == must_hit, where
        if must_hit and end == total:
            assert len(inside) >= 2, where
        found, res, ev = gpu.scan_pool(k, st, target, mask, begin, end,
                                       seed=orc.SCAN_SEED)
        assert found == must_hit, where
        if not found:
            assert ev == end - begin, where
            continue
        assert 1 <= ev <= end - begin, where
        first = inside[0]
        assert orc.hit_ids(k, res) == ref[first][0], (where, first, list(res))
        assert tuple(res) == ref[first][3], (where, first, list(res))
    return len(windows)


@pytest.mark.parametrize("case", CASES[3] + CASES[5] + CASES[7],
                         ids=orc.case_id)
def test_lut_scan_windows(lut_gpu, case):
    check_case_windows(lut_gpu, case)


@pytest.mark.parametrize("case", CASES[4], ids=orc.case_id)
def test_scan4_service_windows(monkeypatch, capfd, case):
    # The engine decides between service and one-shot kernel on its first
    # k=4 scan, from the environment as it is then.
    monkeypatch.delenv("SBOXGATES_NO_SVC", raising=False)
    gpu = ordered_gpu(False, try_nots=True)
    scans = check_case_windows(gpu, case)
    stats = gpu.stats()
    assert stats["gpu_scans"] == scans and stats["cpu_scans"] == 0
    # A service that fails hands its engine to the one-shot kernel and says
    # so; that must not be how this test passed.
    assert "scan service disabled" not in capfd.readouterr().err


@pytest.mark.parametrize("case", CASES[4], ids=orc.case_id)
def test_scan4_oneshot_windows(monkeypatch, case):
    monkeypatch.setenv("SBOXGATES_NO_SVC", "1")
    gpu = ordered_gpu(False, try_nots=True)
    scans = check_case_windows(gpu, case)
    stats = gpu.stats()
    assert stats["gpu_scans"] == scans and stats["cpu_scans"] == 0


# --- 2. and 3. pool 48: the 5-LUT wide walk and the shared-input scan -----------

POOL48 = 48
assert POOL48 - 3 > _core.SCAN5_WIDE_MIN_ROW  # k_scan5<true> runs


def pool48_setup(size):
    eng = orc.cpu_engine(5)
    st = eng.initial_state()
    st.grow_pool_random(POOL48, orc.POOL_SEED + POOL48)
    assert st.num_gates == POOL48
    target = eng.target(0)
    return st, target, orc.sparse_mask(5000 + POOL48 + size, size, target)


def scan_of(eng, kind):
    """scan(st, target, mask, begin, end, excl) -> (found, res, evaluated) of
    the 5-LUT scan (kind 5) or the shared-input scan (kind 4) on eng."""
    def scan(st, target, mask, begin, end, excl=0):
        if kind == 5:
            return eng.scan_pool(5, st, target, mask, begin, end,
                                 seed=orc.SCAN_SEED, excl=excl)
        return eng.scan_shared(st, target, mask, begin, end,
                               seed=orc.SCAN_SEED, excl=excl)
    return scan


def hit_rank(kind, res):
    ids = sorted(res[2:7]) if kind == 5 else sorted(res[2:6])
    return orc.checked_rank(ids, POOL48), ids


def check_pool48(gpu, kind, size, first_hits):
    st, target, mask = pool48_setup(size)
    total = math.comb(POOL48, kind)
    cpu = scan_of(orc.cpu_engine(5), kind)
    dev = scan_of(gpu, kind)
    # The hits in rank order, from the CPU scan restarted behind each hit.
    hits, ids0 = [], None
    begin = 0
    while len(hits) < FIRST_HITS + 2:
        found, res, _ = cpu(st, target, mask, begin, total)
        if not found:
            break
        r, ids = hit_rank(kind, res)
        assert begin <= r < total
        ids0 = ids0 or ids
        hits.append(r)
        begin = r + 1
    assert len(hits) >= FIRST_HITS + 2, hits
    assert hits[:len(first_hits)] == first_hits
    windows = [(0, total, 0)] + [(h + 1, total, 0) for h in hits[:FIRST_HITS]]
    # The ids of the first hit excluded (all below 64): the hit moves.
    excl = sum(1 << g for g in ids0)
    windows.append((0, total, excl))
    for begin, end, ex in windows:
        where = (kind, size, begin, end, ex)
        f_c, r_c, ev_c = cpu(st, target, mask, begin, end, ex)
        f_g, r_g, ev_g = dev(st, target, mask, begin, end, ex)
        assert f_g == f_c, where
        if not f_c:
            assert ev_g == ev_c, where
            continue
        assert list(r_g) == list(r_c), where
        assert 1 <= ev_g <= end - begin, where
        if ex:
            assert hit_rank(kind, r_c)[0] != hits[0], where


@pytest.mark.parametrize("size,first_hits", [
    (20, [1642, 15325, 15327, 15328]),
    (24, [157811, 252250, 254055, 382218, 384023, 624275, 905988]),
])
def test_scan5_wide_walk_windows(lut_gpu, size, first_hits):
    check_pool48(lut_gpu, 5, size, first_hits)


@pytest.mark.parametrize("size,first_hits", [
    (16, [120, 918, 2088, 2101]),
    (20, [50099, 51418, 52137]),
])
def test_shared_scan_windows(lut_gpu, size, first_hits):
    check_pool48(lut_gpu, 4, size, first_hits)


# --- 4. 7-LUT with range splitting --------------------------------------------

DEEP7_TOTAL = math.comb(orc.DEEP7_POOL, 7)
DEEP7_HITS = (orc.DEEP7_FIRST, 109168, 133022)
DEEP7_WINDOWS = ((0, DEEP7_TOTAL), (DEEP7_HITS[0] + 1, DEEP7_TOTAL),
                 (DEEP7_HITS[1] + 1, DEEP7_TOTAL), (0, DEEP7_HITS[0]))


@pytest.fixture(scope="module")
def deep7_cpu():
    """cpu_scan7 on every deep window, once."""
    st, target, mask = orc.deep7_setup()
    cpu = orc.cpu_engine(7)
    out = [cpu.scan_pool(7, st, target, mask, begin, end, seed=orc.SCAN_SEED)
           for begin, end in DEEP7_WINDOWS]
    ranks = [orc.checked_rank(orc.hit_ids(7, res), orc.DEEP7_POOL)
             for found, res, _ in out if found]
    assert ranks == list(DEEP7_HITS) and not out[3][0]
    return out


def check_deep7(results, expected):
    for (begin, end), got, want in zip(DEEP7_WINDOWS, results, expected):
        where = (begin, end)
        assert bool(got[0]) == bool(want[0]), where
        if not want[0]:
            assert got[2] == want[2] == end - begin, where
            continue
        assert list(got[1]) == list(want[1]), where
        assert 1 <= got[2] <= end - begin, where


def test_scan7_deep_windows(lut_gpu, deep7_cpu):
    st, target, mask = orc.deep7_setup()
    check_deep7([lut_gpu.scan_pool(7, st, target, mask, begin, end,
                                   seed=orc.SCAN_SEED)
                 for begin, end in DEEP7_WINDOWS], deep7_cpu)


def test_scan7_deep_windows_small_cap(lut_gpu, deep7_cpu):
    """The same windows in a fresh process whose hit buffer holds 64 entries,
    so that the scan splits its range: the first sub-range with a hit ends
    the scan, and that hit is the window's lowest."""
    env = dict(os.environ)
    env["SBOXGATES_HIT_CAP"] = "64"
    worker = os.path.join(os.path.dirname(os.path.abspath(__file__)),
                          "_ordered7_worker.py")
    args = ["%d:%d" % w for w in DEEP7_WINDOWS]
    r = subprocess.run([sys.executable, worker] + args, env=env,
                       capture_output=True, text=True, timeout=90)
    assert r.returncode == 0, r.stderr
    results = json.loads(r.stdout.strip().splitlines()[-1])
    assert len(results) == len(args)
    check_deep7(results, deep7_cpu)


# --- 5. whole searches --------------------------------------------------------

def check_scanned_on_gpu(stats, where):
    if stats["gpu_scans"] + stats["cpu_scans"] > 0:
        assert stats["gpu_scans"] > 0 and stats["cpu_scans"] == 0, (where, stats)


@pytest.mark.parametrize("case", sorted(pinned.CIRCUIT_CASES))
def test_forced_gpu_search_reproduces_pins(case):
    if not _core.gpu_available():
        pytest.skip("no GPU")
    got, stats = test_ordered.run_ordered_circuit(case, "force")
    want = pinned.load_pins()["create_circuit"][case]
    for key in ("xml_sha256", "gates", "nodes"):
        assert got[key] == want[key], (case, key, got, want)
    check_scanned_on_gpu(stats, case)
    if case == "lut":
        again, _ = test_ordered.run_ordered_circuit(case, "force")
        assert again["xml_sha256"] == got["xml_sha256"]


def test_forced_gpu_shared_search_equals_cpu():
    if not _core.gpu_available():
        pytest.skip("no GPU")
    from sboxgates_amd import models
    from sboxgates_amd.ops import make_engine, mask_for_inputs
    sbox, n = models.load("des_s1")
    xml = {}
    for gpu in ("off", "force"):
        eng = make_engine(lut_graph=True, lut_shared=True, seed=1, gpu=gpu,
                          ordered=gpu == "force", save_states=False)
        eng.set_sbox(sbox, n)
        st = eng.initial_state()
        out = eng.create_circuit(st, eng.target(0), mask_for_inputs(n))
        assert out >= 0
        st.set_output(0, out)
        stats = eng.stats()
        assert stats["shared_hits"] > 0
        xml[gpu] = (st.to_xml(), stats["nodes"], stats["shared_hits"])
        if gpu == "force":
            check_scanned_on_gpu(stats, "lut_shared")
            assert stats["gpu_scans"] > 0
    assert xml["force"] == xml["off"]
