"""Window handling of GpuEngine::scan, per scan kind: empty windows, windows
past the end of the combination space, windows that straddle it and, for
the two kinds whose CPU scans clamp it, a negative begin. The GPU engine
must report what the CPU engine reports on the same call.

Pool: 10 gates (8 inputs + 2 random), AES bit-0 target, full mask, no
exclusions, so a count_all scan of a window evaluates exactly the ranks of
the window that exist: 0, 0, 3 and T for the four windows below (derived,
not measured).
"""

import pytest

import _oracle as orc
from sboxgates_amd import _core
from sboxgates_amd.ops import mask_for_inputs, n_choose_k

pytestmark = pytest.mark.gpu

POOL = 10
POOL_SEED = 0xA0 + POOL


def make_pool(engine):
    st = engine.initial_state()
    st.grow_pool_random(POOL, POOL_SEED)
    return st


def windows(total):
    """(begin, end, evaluated by a count_all scan)."""
    return [(0, 0, 0), (total, total + 7, 0), (total - 3, total + 7, 3),
            (0, total + 7, total)]


def scan_counting(kind):
    """The count_all scan of `kind` as f(engine, st, begin, end)."""
    def scan(eng, st, begin, end):
        target, mask = eng.target(0), mask_for_inputs(8)
        if kind == "shared":
            return eng.scan_shared(st, target, mask, begin, end,
                                   seed=orc.SCAN_SEED, count_all=True)
        return eng.scan_pool(kind, st, target, mask, begin, end,
                             seed=orc.SCAN_SEED, count_all=True)
    return scan


def check_counting(gpu, cpu, kind, comb_k):
    scan = scan_counting(kind)
    st = make_pool(gpu)
    total = n_choose_k(POOL, comb_k)
    for begin, end, evaluated in windows(total):
        f_g, _, ev_g = scan(gpu, st, begin, end)
        f_c, _, ev_c = scan(cpu, st, begin, end)
        where = (kind, begin, end)
        assert (f_g, ev_g) == (f_c, ev_c), where
        assert ev_c == evaluated, where
    return st


def check_pairs(gpu, cpu):
    st = make_pool(gpu)
    target, mask = gpu.target(0), mask_for_inputs(8)
    total = n_choose_k(POOL, 2)

    def scan(eng, begin, end):
        found, res, ev = eng.scan_pairs(st, target, mask, begin, end)
        return found, tuple(res), ev

    for begin, end, _ in windows(total) + [(-5, 3, None)]:
        assert scan(gpu, begin, end) == scan(cpu, begin, end), (begin, end)
    assert scan(gpu, -5, 3) == scan(cpu, 0, 3)


def assert_all_on_gpu(gpu):
    stats = gpu.stats()
    assert stats["cpu_scans"] == 0 and stats["pair_scans_cpu"] == 0
    assert stats["gpu_scans"] + stats["pair_scans_gpu"] > 0


@pytest.fixture(scope="module")
def lut_engines():
    if not _core.gpu_available():
        pytest.skip("no GPU")
    gpu, cpu = orc.make_pair(True)
    assert gpu.gpu_active
    return gpu, cpu


@pytest.mark.parametrize("kind,comb_k", [(3, 3), (5, 5), (7, 7), ("shared", 4)])
def test_lut_windows(lut_engines, kind, comb_k):
    gpu, cpu = lut_engines
    st = check_counting(gpu, cpu, kind, comb_k)
    if kind == "shared":
        # cpu_scan4s clamps a negative begin; so must the GPU engine.
        scan = scan_counting(kind)
        got, want = scan(gpu, st, -5, 3), scan(cpu, st, -5, 3)
        assert (got[0], got[2]) == (want[0], want[2]) == (False, 3)
        assert (got[0], got[2]) == scan(gpu, st, 0, 3)[::2]
    assert_all_on_gpu(gpu)


def gate_engines():
    """A fresh pair: the GPU engine decides between service and one-shot
    kernels on its first gate-mode scan, from the environment as it is then."""
    if not _core.gpu_available():
        pytest.skip("no GPU")
    gpu, cpu = orc.make_pair(False, try_nots=True)
    assert gpu.gpu_active
    return gpu, cpu


def test_gate_windows_service(monkeypatch, capfd):
    monkeypatch.delenv("SBOXGATES_NO_SVC", raising=False)
    gpu, cpu = gate_engines()
    check_counting(gpu, cpu, 4, 3)
    check_pairs(gpu, cpu)
    assert_all_on_gpu(gpu)
    # A service that fails hands its engine to the one-shot kernels and says
    # so; that must not be how this test passed.
    assert "scan service disabled" not in capfd.readouterr().err


def test_gate_windows_oneshot(monkeypatch):
    monkeypatch.setenv("SBOXGATES_NO_SVC", "1")
    gpu, cpu = gate_engines()
    check_counting(gpu, cpu, 4, 3)
    check_pairs(gpu, cpu)
    assert_all_on_gpu(gpu)
