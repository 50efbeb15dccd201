"""State the persistent k=4 scan service keeps across requests, sequenced on
purpose: the pinned pool shadow and its `keep` delta (a pool that grows, an
unrelated shorter pool, the first pool again), the matcher epoch (two
engines with different function lists sharing the one service per device),
the device pool that survives a park by a k=5 scan, and, in a child
process with a short idle limit, retire and relaunch."""

import math
import os
import random
import subprocess
import sys

import pytest

import _oracle as orc
from sboxgates_amd import _core
from sboxgates_amd.ops import function_lists, gen_lut_ttable, mask_for_inputs

pytestmark = pytest.mark.gpu

FULL = mask_for_inputs(8)
# Engine A: the default gate set; engine B: AND and XOR only. Both with NOT
# gates, which is what gives them 3-input function lists.
GATES_A = orc.GATE_BITFIELD
GATES_B = 2 + 64


def make_pools(eng):
    p1 = eng.initial_state()
    p1.grow_pool_random(40, 0xD1)
    grown = p1.copy()
    grown.grow_pool_random(60, 0xD2)
    other = eng.initial_state()
    other.grow_pool_random(30, 0xD3)
    assert (p1.num_gates, grown.num_gates, other.num_gates) == (40, 60, 30)
    tab = lambda st, i: st.gate(i)["table"]
    # The grown pool keeps P1's 40 gates; the unrelated one shares only the
    # 8 inputs with it.
    assert all(tab(p1, i) == tab(grown, i) for i in range(40))
    assert all(tab(p1, i) == tab(other, i) for i in range(8))
    assert tab(p1, 8) != tab(other, 8)
    return {"p1": p1, "grown": grown, "other": other}


def check_step(step, gpu, cpu, threes, st):
    """One planted full-range window and 50 single-rank windows under a
    6-position mask, against the CPU engine and the oracle."""
    n = st.num_gates
    total = math.comb(n, 3)
    assert total <= 1 << 20          # the service serves requests this small
    rng = random.Random(0x5E0 + step)
    funs = [f["fun"] for f in threes]
    tabs = [st.gate(i)["table"] for i in range(n)]
    itabs = [orc.tt_int(t) for t in tabs]
    full = orc.tt_int(FULL)

    # Planted: some triple realises the target, so the verdict is "found".
    while True:
        ids = sorted(rng.sample(range(n), 3))
        target = gen_lut_ttable(rng.choice(funs), *(tabs[i] for i in ids))
        if 0 < orc.tt_int(target) & full < full:
            break
    orc.assert_mask_has_target1(target, FULL)
    assert orc.found4([itabs[i] for i in ids], orc.tt_int(target), full,
                      funs) is not None
    f_g, r_g, _ = gpu.scan_pool(4, st, target, FULL, 0, total, seed=step)
    f_c, r_c, _ = cpu.scan_pool(4, st, target, FULL, 0, total, seed=step)
    assert f_g and f_c, step
    orc.assert_hit_valid(4, st, r_g, target, FULL, threes)
    _, _, ev_g = gpu.scan_pool(4, st, target, FULL, 0, total, seed=step,
                               count_all=True)
    assert ev_g == total, step

    # Single ranks under a sparse mask: verdict, result words, validity.
    target = gpu.target(0)
    mask = orc.sparse_mask(0x5E00 + step, 6, target)
    t, m = orc.tt_int(target), orc.tt_int(mask)
    hits = 0
    for r in rng.sample(range(total), 50):
        comb = orc.checked_unrank(r, n, 3)
        verdict = orc.found4([itabs[i] for i in comb], t, m, funs)
        f_g, r_g, ev_g = gpu.scan_pool(4, st, target, mask, r, r + 1,
                                       seed=step)
        f_c, r_c, _ = cpu.scan_pool(4, st, target, mask, r, r + 1, seed=step)
        where = (step, r, comb)
        assert ev_g == 1, where
        assert f_g == f_c == (verdict is not None), where
        if f_g:
            hits += 1
            assert list(r_g) == list(r_c), where
            assert (r_g[0], r_g[1]) == verdict, where
            assert orc.hit_ids(4, r_g) == comb, where
            orc.assert_hit_valid(4, st, r_g, target, mask, threes)
    return hits


def run_sequence(pair_a, pair_b):
    threes_a = function_lists(GATES_A, True)[2]
    threes_b = function_lists(GATES_B, True)[2]
    funs_a = [f["fun"] for f in threes_a]
    funs_b = [f["fun"] for f in threes_b]
    assert funs_a and funs_b and funs_a != funs_b
    a = pair_a + (threes_a,)
    b = pair_b + (threes_b,)
    pools = make_pools(pair_a[1])

    hits = 0
    sequence = [("p1", a), ("grown", b), "park", ("other", a), ("p1", b),
                ("grown", a), ("other", b), "park", ("p1", a)]
    for step, item in enumerate(sequence):
        if item == "park":
            # A k=5 scan on a GPU engine that holds the service parks it;
            # the next k=4 request has to relaunch it over the device pool
            # left behind.
            gpu, cpu = pair_a[:2]
            st = pools["other"]
            args = (5, st, gpu.target(0), FULL, 0, 5000)
            assert (gpu.scan_pool(*args, count_all=True)[2] ==
                    cpu.scan_pool(*args, count_all=True)[2] == 5000)
            continue
        name, (gpu, cpu, threes) = item
        hits += check_step(step, gpu, cpu, threes, pools[name])
    return hits


def test_service_state_sequence(monkeypatch, capfd):
    if not _core.gpu_available():
        pytest.skip("no GPU")
    monkeypatch.delenv("SBOXGATES_NO_SVC", raising=False)
    pair_a = orc.make_pair(False, try_nots=True, gate_bitfield=GATES_A)
    pair_b = orc.make_pair(False, try_nots=True, gate_bitfield=GATES_B)
    assert pair_a[0].gpu_active and pair_b[0].gpu_active
    hits = run_sequence(pair_a, pair_b)
    # The single-rank windows were not all misses (38 hits on the CPU).
    assert hits >= 10
    for gpu in (pair_a[0], pair_b[0]):
        assert gpu.stats()["cpu_scans"] == 0
    # No fall-back from a failed service to the one-shot kernel.
    assert "scan service disabled" not in capfd.readouterr().err


def test_engine_teardown_stops_service_first(monkeypatch):
    """An engine frees its device buffers when it is destroyed, and hipFree
    waits for every kernel on the device. With the service kernel still
    resident that wait lasted until the kernel's idle limit: 1.77 s per
    engine, measured. The engine now stops the service before it frees.

    Bound: the stop handshake is a few polls of a pinned word and the frees
    take milliseconds, while the idle limit is 500000 polls of two PCIe
    reads and an s_sleep each, which cannot finish in under a second. 0.5 s
    separates the two with room on both sides."""
    import time
    if not _core.gpu_available():
        pytest.skip("no GPU")
    monkeypatch.delenv("SBOXGATES_NO_SVC", raising=False)
    gpu, cpu = orc.make_pair(False, try_nots=True)
    st = gpu.initial_state()
    st.grow_pool_random(24, 5)
    args = (4, st, gpu.target(0), FULL, 0, math.comb(24, 3))
    assert (gpu.scan_pool(*args, count_all=True)[2] ==
            cpu.scan_pool(*args, count_all=True)[2] == math.comb(24, 3))
    t0 = time.perf_counter()
    del gpu
    dt = time.perf_counter() - t0
    print(f"engine teardown with the service resident: {dt * 1e3:.1f} ms")
    assert dt < 0.5


RETIRE_CHILD = r'''
import math
import sys
import time
sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import random
import _oracle as orc
from sboxgates_amd.ops import gen_lut_ttable, mask_for_inputs

gpu, cpu = orc.make_pair(False, try_nots=True)
assert gpu.gpu_active
threes = orc.threes_default()
mask = mask_for_inputs(8)
pools = []
for n, seed in ((40, 0xE1), (30, 0xE2)):
    st = gpu.initial_state()
    st.grow_pool_random(n, seed)
    pools.append(st)
rng = random.Random(0xE3)


def scan(st):
    n = st.num_gates
    total = math.comb(n, 3)
    ids = sorted(rng.sample(range(n), 3))
    target = gen_lut_ttable(rng.choice(threes)["fun"],
                            *(st.gate(i)["table"] for i in ids))
    r = orc.checked_rank(ids, n)
    f_g, r_g, ev_g = gpu.scan_pool(4, st, target, mask, r, r + 1)
    f_c, r_c, ev_c = cpu.scan_pool(4, st, target, mask, r, r + 1)
    assert (f_g, list(r_g), ev_g) == (f_c, list(r_c), ev_c), (ids, r_g, r_c)
    if f_g:
        orc.assert_hit_valid(4, st, r_g, target, mask, threes)
    _, _, ev_g = gpu.scan_pool(4, st, gpu.target(0), mask, 0, total,
                               count_all=True)
    assert ev_g == total


for _ in range(3):
    scan(pools[0])
    time.sleep(0.5)
    scan(pools[1])
assert gpu.stats()["cpu_scans"] == 0
print("retire-relaunch ok")
'''


def test_service_retire_and_relaunch():
    """SBOXGATES_SVC_IDLE is read once per process, so a child process gets
    an idle limit of 1000 polls (a few milliseconds): the service retires
    during each 0.5 s pause and the next request relaunches it over the
    device pool of the request before. The launch lines in the child's
    debug output prove that it did retire."""
    if not _core.gpu_available():
        pytest.skip("no GPU")
    env = dict(os.environ)
    env.pop("SBOXGATES_NO_SVC", None)
    env["SBOXGATES_SVC_IDLE"] = "1000"
    env["SBOXGATES_SVC_DEBUG"] = "1"
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", RETIRE_CHILD], env=env,
                       capture_output=True, text=True, timeout=120, cwd=repo)
    assert r.returncode == 0, r.stderr
    assert "retire-relaunch ok" in r.stdout
    assert "scan service disabled" not in r.stderr
    launches = [ln for ln in r.stderr.splitlines()
                if ln.startswith("[svc] launch #")]
    assert len(launches) >= 2, r.stderr
