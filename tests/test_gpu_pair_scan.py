"""The GPU pair scan (k=2) against the CPU pair scan and the independent
oracle of tests/_oracle_pairs.py, on the persistent scan service and on the
one-shot k_scan2 kernel: per-rank verdicts, the lowest-rank election over
full windows (the answer is deterministic, so result words and `evaluated`
are compared exactly), the state the service keeps across alternating k=4
and k=2 requests, the gpu_pairs routing of create_circuit, and a whole
search in a child process.
"""

import math
import os
import random
import subprocess
import sys

import pytest

import _oracle as orc
import _oracle_pairs as op
from sboxgates_amd import _core
from sboxgates_amd.ops import mask_for_inputs, scan_pairs

pytestmark = pytest.mark.gpu

CASES = [(s, w) for s in op.MASK_SIZES for w in op.LISTS]
PATHS = ["service", "oneshot"]
FULL = mask_for_inputs(8)


def case_id(case):
    return "mask%d-%s" % case


def fresh_gpu(monkeypatch, path, bitfield=op.GATE_BITFIELD, **kw):
    """A gpu="force" engine that decides between the service and the one-shot
    kernel on its first scan, from the environment as it is then."""
    if not _core.gpu_available():
        pytest.skip("no GPU")
    if path == "service":
        monkeypatch.delenv("SBOXGATES_NO_SVC", raising=False)
    else:
        monkeypatch.setenv("SBOXGATES_NO_SVC", "1")
    gpu = op.rijndael_engine(gpu="force", bitfield=bitfield, **kw)
    assert gpu.gpu_active
    return gpu


def check_stats(gpu, scans, capfd):
    stats = gpu.stats()
    assert stats["pair_scans_gpu"] == scans and stats["pair_scans_cpu"] == 0
    assert stats["gpu_scans"] == 0 and stats["cpu_scans"] == 0
    # A service that fails hands its engine to the one-shot kernel and says
    # so; that must not be how a test passed.
    assert "scan service disabled" not in capfd.readouterr().err


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_per_rank(monkeypatch, capfd, case, path):
    size, which = case
    gpu = fresh_gpu(monkeypatch, path)
    cpu = op.cpu_engine()
    st, target, mask = op.case_setup(size)
    funs = op.fun_lists()[which]
    scans = 0
    for order_name, order in op.orders(op.POOL).items():
        verdicts = op.case_verdicts(size, which, order_name)
        arg = None if order_name == "identity" else order
        for r, verdict in enumerate(verdicts):
            got = scan_pairs(gpu, st, target, mask, r, r + 1, which, arg)
            ref = scan_pairs(cpu, st, target, mask, r, r + 1, which, arg)
            scans += 1
            where = (case, path, order_name, r)
            assert (got[0], list(got[1]), got[2]) == (
                ref[0], list(ref[1]), ref[2]), where
            assert got[2] == 1, where
            assert got[0] == (verdict is not None), where
            if got[0]:
                i, k = op.pair_of_rank(r, op.POOL)
                assert tuple(got[1][:4]) == op.expected(
                    verdict, order[i], order[k]), where
                op.assert_hit_valid(st, funs, got[1], target, mask)
    check_stats(gpu, scans, capfd)


def election_windows(cpu, st, target, mask, which, order):
    """Full window, windows that start just after each of the first hits,
    and a window inside the gap before the first hit (a miss)."""
    total = math.comb(st.num_gates, 2)
    hits = op.cpu_hits(cpu, st, target, mask, which, order, 3)
    assert len(hits) == 3
    out = [(0, total), (17, total - 5)] + [(h + 1, total) for h in hits]
    if hits[0] > 0:
        out.append((0, hits[0]))                    # miss
    out.append((hits[0] + 1, hits[1]))              # miss, possibly empty
    return out


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("n", [24, 200, 500])
def test_lowest_rank_election(monkeypatch, capfd, n, path):
    """Pool 24 under the 3-position mask: 140 hits over two workgroups. Pool
    200: 19,900 ranks, past the service's 16,384 threads, so the stride loop
    runs. Pool 500: MAX_GATES."""
    gpu = fresh_gpu(monkeypatch, path)
    cpu = op.cpu_engine()
    if n == 24:
        st, target, mask = op.case_setup(3)
        order = op.orders(24)["shuffled"]
    else:
        st, target, mask, order = op.big_pool(n)
        order = list(order)
    scans = 0
    misses = 0
    for which in op.LISTS:
        funs = op.fun_lists()[which]
        for begin, end in election_windows(cpu, st, target, mask, which, order):
            got = scan_pairs(gpu, st, target, mask, begin, end, which, order)
            ref = scan_pairs(cpu, st, target, mask, begin, end, which, order)
            scans += 1
            where = (n, path, which, begin, end)
            assert (got[0], list(got[1]), got[2]) == (
                ref[0], list(ref[1]), ref[2]), where
            if got[0]:
                op.assert_hit_valid(st, funs, got[1], target, mask)
            elif end > begin:
                misses += 1
                assert got[2] == end - begin, where
    assert misses >= 1
    check_stats(gpu, scans, capfd)


def test_service_state_alternating_k4_k2(monkeypatch, capfd):
    """One service, two engines with different gate sets, k=4 and k=2
    requests in turn over a pool that grows, an unrelated shorter pool and
    the first pool again, a k=5 scan in between to park the service, and
    another order on every k=2 request."""
    a = fresh_gpu(monkeypatch, "service", bitfield=214)
    b = fresh_gpu(monkeypatch, "service", bitfield=194)
    cpus = {id(a): op.cpu_engine(214), id(b): op.cpu_engine(194)}
    p1 = a.initial_state()
    p1.grow_pool_random(40, 0xD1)
    grown = p1.copy()
    grown.grow_pool_random(60, 0xD2)
    other = a.initial_state()
    other.grow_pool_random(30, 0xD3)
    pools = {"p1": p1, "grown": grown, "other": other}
    assert (p1.num_gates, grown.num_gates, other.num_gates) == (40, 60, 30)
    target = a.target(0)
    rng = random.Random(0x2A4)
    sequence = [("p1", a), ("grown", b), "park", ("other", a), ("p1", b),
                ("grown", a), ("other", b), "park", ("p1", a)]
    pair_scans = {id(a): 0, id(b): 0}
    k4_scans = {id(a): 0, id(b): 0}
    found_pairs = 0
    for step, item in enumerate(sequence):
        if item == "park":
            args = (5, other, target, FULL, 0, 5000)
            assert a.scan_pool(*args, count_all=True)[2] == 5000
            k4_scans[id(a)] += 1
            continue
        name, gpu = item
        cpu = cpus[id(gpu)]
        st = pools[name]
        n = st.num_gates
        total3 = math.comb(n, 3)
        mask = orc.sparse_mask(0x5E00 + step, 4, target)
        for sub in range(3):
            # k=4: single-rank windows (their winner is no race) and a count.
            r = rng.randrange(total3)
            got = gpu.scan_pool(4, st, target, mask, r, r + 1, seed=step)
            ref = cpu.scan_pool(4, st, target, mask, r, r + 1, seed=step)
            assert (got[0], list(got[1]), got[2]) == (
                ref[0], list(ref[1]), ref[2]), (step, sub, r)
            k4_scans[id(gpu)] += 1
            # k=2: the whole window and a later one, under a fresh order.
            order = list(range(n))
            rng.shuffle(order)
            begin = rng.randrange(math.comb(n, 2) // 2)
            for which in op.LISTS:
                for lo in (0, begin):
                    got = scan_pairs(gpu, st, target, mask, lo, 10 ** 6, which,
                                     order)
                    ref = scan_pairs(cpu, st, target, mask, lo, 10 ** 6, which,
                                     order)
                    assert (got[0], list(got[1]), got[2]) == (
                        ref[0], list(ref[1]), ref[2]), (step, sub, which, lo)
                    pair_scans[id(gpu)] += 1
                    found_pairs += got[0]
        assert gpu.scan_pool(4, st, target, FULL, 0, total3,
                             count_all=True)[2] == total3
        k4_scans[id(gpu)] += 1
    assert found_pairs >= 10
    for gpu in (a, b):
        stats = gpu.stats()
        assert stats["pair_scans_gpu"] == pair_scans[id(gpu)]
        assert stats["gpu_scans"] == k4_scans[id(gpu)]
        assert stats["cpu_scans"] == 0 and stats["pair_scans_cpu"] == 0
    assert "scan service disabled" not in capfd.readouterr().err


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("which", op.LISTS)
def test_routing_planted(monkeypatch, capfd, which, path):
    """create_circuit with gpu_pairs="force" sends its pair sweeps through
    the GPU pair scan and builds the circuit of a gpu="off" engine."""
    gpu = fresh_gpu(monkeypatch, path, gpu_pairs="force")
    cpu = op.rijndael_engine()
    xml_gpu = op.check_planted_circuit(gpu, which).to_xml()
    xml_cpu = op.check_planted_circuit(cpu, which).to_xml()
    assert xml_gpu == xml_cpu
    stats = gpu.stats()
    assert stats["pair_scans_gpu"] == (1 if which == "gates" else 2)
    assert stats["pair_scans_cpu"] == 0
    assert cpu.stats()["pair_scans_gpu"] == 0
    assert "scan service disabled" not in capfd.readouterr().err


def test_routing_auto_cutover(monkeypatch, capfd):
    """gpu_pairs="auto" keeps the host sweep below the cutover (170 gates)
    and sends the sweeps of a larger pool to the GPU, with the same result:
    a node whose step 3 misses and whose bounds end it before step 4a."""
    if not _core.gpu_available():
        pytest.skip("no GPU")
    monkeypatch.delenv("SBOXGATES_NO_SVC", raising=False)
    auto = op.rijndael_engine(gpu="auto", gpu_pairs="auto")
    off = op.rijndael_engine(gpu="off")
    xml = op.check_planted_circuit(auto, "gates").to_xml()
    assert xml == op.check_planted_circuit(off, "gates").to_xml()
    assert auto.stats()["pair_scans_gpu"] == 0
    expect = 0
    for n in (169, 170, 200):
        st = auto.initial_state()
        st.grow_pool_random(n, orc.POOL_SEED + n)
        st.max_gates = n + 1
        assert auto.create_circuit(st, auto.target(0), FULL) == -1
        assert st.num_gates == n
        expect += n >= 170
        assert auto.stats()["pair_scans_gpu"] == expect, n
    assert auto.stats()["pair_scans_cpu"] == 0
    assert "scan service disabled" not in capfd.readouterr().err


SEARCH_CHILD = r'''
import sys
sys.path.insert(0, ".")
from sboxgates_amd import _core, models
from sboxgates_amd.ops import make_engine
from sboxgates_amd.utils import validate_circuit

sbox, n = models.load("des_s1")
out = {}
for name, kw in (("gpu", dict(gpu="auto", gpu_pairs="force")),
                 ("cpu", dict(gpu="off"))):
    eng = make_engine(lut_graph=False, seed=5, try_nots=True,
                      gate_bitfield=214, save_states=False, **kw)
    eng.set_sbox(sbox, n)
    st = eng.initial_state()
    g = eng.create_circuit(st, eng.target(0), _core.mask_for_inputs(n))
    assert g >= 0
    st.set_output(0, g)
    assert validate_circuit(st, sbox, n, bit=0)
    out[name] = (st.to_xml(), eng.stats())
assert out["gpu"][1]["pair_scans_gpu"] > 0, out["gpu"][1]
assert out["gpu"][1]["pair_scans_cpu"] == 0
assert out["cpu"][1]["pair_scans_gpu"] == 0
assert out["gpu"][0] == out["cpu"][0], "circuits differ"
print("pair scans on the GPU:", out["gpu"][1]["pair_scans_gpu"],
      "nodes:", out["gpu"][1]["nodes"])
print("whole-search ok")
'''


def test_whole_search_identical():
    """DES S1 output 0 in gate mode, seeded, once with every pair sweep on
    the GPU and once on the host: the same circuit. A child process, because
    SBOXGATES_GPU_MIN4 is read once per process; it keeps the k=4 scans,
    whose winner is a race on the GPU, on the CPU."""
    if not _core.gpu_available():
        pytest.skip("no GPU")
    env = dict(os.environ)
    env.pop("SBOXGATES_NO_SVC", None)
    env["SBOXGATES_GPU_MIN4"] = "2000000000"
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", SEARCH_CHILD], env=env,
                       capture_output=True, text=True, timeout=120, cwd=repo)
    assert r.returncode == 0, r.stderr
    assert "whole-search ok" in r.stdout
    assert "scan service disabled" not in r.stderr
