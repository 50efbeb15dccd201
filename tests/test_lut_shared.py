"""The shared-input two-LUT scan (options.lut_shared) on the CPU path: the
solver against brute force, cpu_scan4s per rank against the independent
oracle of tests/_oracle_shared.py, the planted search that needs the scan,
the inert option, and the round trip of a state whose LUT pair shares an
input.

Hits and shares of the per-rank cases, from the oracle (pool, mask size):
(12, 8) 75 of 495; (12, 10) 34 of 495; (16, 8) 535 of 1820; (16, 10) 301 of
1820.
"""

import os
import random
import subprocess

import pytest

import _oracle as orc
import _oracle_shared as osh
from conftest import rand_tt
from sboxgates_amd import _core, models
from sboxgates_amd.ops import (gen_lut_ttable, graph_to_source, lut4s_solve,
                               make_engine, scan_shared, tt_eq_mask)
from sboxgates_amd.utils import validate_circuit

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(REPO, "bin", "sboxgates")


# --- 1. solver against brute force -------------------------------------------

def test_solver_against_brute_force():
    rng = random.Random(0x4515)
    found = missed = 0
    shapes = set()
    for i in range(400):
        tabs = [rand_tt(rng) for _ in range(4)]
        if i % 2 == 0:
            target = rand_tt(rng)
            size = rng.choice((5, 6, 7, 8, 10, 12))
        else:
            # Planted in a random shape, under a mask large enough that few
            # other shapes fit: the solver has to reach the later ones.
            triple, r, s = osh.shape_positions(rng.randrange(12))
            t_o = gen_lut_ttable(rng.randrange(1, 256),
                                 *(tabs[j] for j in triple))
            target = gen_lut_ttable(rng.randrange(1, 256), t_o, tabs[r],
                                    tabs[s])
            size = rng.choice((24, 32, 48))
        while True:
            pos = rng.sample(range(256), size)
            mask = orc.tt_bytes(sum(1 << p for p in pos))
            if orc.tt_int(mask) & orc.tt_int(target):
                break
        want = osh.found4s([orc.tt_int(t) for t in tabs], orc.tt_int(target),
                           orc.tt_int(mask))
        got = lut4s_solve(tabs, target, mask, rng.getrandbits(64))
        assert (got is not None) == want, (i, got, want)
        if got is None:
            missed += 1
            continue
        found += 1
        fo, fi, shape = got
        assert 0 <= shape < 12 and fo != 0 and fi != 0, got
        shapes.add(shape)
        triple, r, s = osh.shape_positions(shape)
        t_o = gen_lut_ttable(fo, *(tabs[j] for j in triple))
        assert tt_eq_mask(target, gen_lut_ttable(fi, t_o, tabs[r], tabs[s]),
                          mask), (i, got)
    # Neither verdict may be the only one seen, and later shapes are reached.
    assert found >= 40 and missed >= 40, (found, missed)
    assert len(shapes) >= 6, shapes


# --- 2. cpu_scan4s per rank against the oracle -------------------------------

@pytest.mark.parametrize("case", osh.SHARED_CASES, ids=osh.case_id)
def test_cpu_scan4s_per_rank(case):
    st, target, mask, total = osh.case_setup(case)
    orc.assert_mask_has_target1(target, mask)
    ref = osh.case_reference(case)
    assert len(ref) == total
    eng = orc.cpu_engine(5)
    hits = beyond3 = 0
    for r, (comb, verdict, sub3, f_c, r_c) in enumerate(ref):
        assert f_c == verdict, (osh.case_id(case), r, comb)
        excluded = any(g < 64 and (osh.EXCL >> g) & 1 for g in comb)
        f_x, r_x, ev_x = scan_shared(eng, st, target, mask, r, r + 1,
                                     seed=orc.SCAN_SEED, excl=osh.EXCL)
        if excluded:
            # Neither reported nor counted.
            assert (f_x, ev_x) == (False, 0), (r, comb)
        else:
            assert (f_x, tuple(r_x), ev_x) == (f_c, r_c, 1), (r, comb)
        if not f_c:
            continue
        hits += 1
        beyond3 += 0 if sub3 else 1
        osh.assert_hit_layout(r_c, comb)
        orc.assert_hit_valid(5, st, r_c, target, mask)
    share = hits / total
    print(f"{osh.case_id(case)}: {hits}/{total} hits ({100 * share:.1f}%), "
          f"{beyond3} with no 3-LUT subset")
    assert 0.02 <= share <= 0.98, share
    assert beyond3 >= 1


def test_cpu_scan4s_windows():
    """A whole-range scan reports a valid hit, count_all counts every
    combination without an excluded gate, and windows clip to the space."""
    case = (12, 8)
    st, target, mask, total = osh.case_setup(case)
    eng = orc.cpu_engine(5)
    ref = osh.case_reference(case)
    found, res, ev = scan_shared(eng, st, target, mask, 0, total + 5,
                                 seed=orc.SCAN_SEED)
    first = next(r for r, row in enumerate(ref) if row[1])
    assert found and ev == first + 1
    assert tuple(res) == ref[first][4]
    found, _, ev = scan_shared(eng, st, target, mask, 0, total, count_all=True)
    assert not found and ev == total
    clean = sum(1 for row in ref
                if not any((osh.EXCL >> g) & 1 for g in row[0]))
    found, _, ev = scan_shared(eng, st, target, mask, 0, total, count_all=True,
                               excl=osh.EXCL)
    assert not found and ev == clean
    assert scan_shared(eng, st, target, mask, total, total + 9)[2] == 0


# --- 3. planted search -------------------------------------------------------

@pytest.mark.parametrize("num_inputs", [4, 6])
def test_planted_search(num_inputs):
    for seed in range(1, 21):
        luts, stats = osh.planted_search(num_inputs, seed, lut_shared=True)
        assert luts == 2 and stats["shared_hits"] == 1, (seed, luts, stats)
        assert stats["candidates4s"] > 0
        luts, stats = osh.planted_search(num_inputs, seed)
        assert luts >= 3 and stats["shared_hits"] == 0, (seed, luts)


# --- 4. option off is inert --------------------------------------------------

def des_bit0(**kw):
    sbox, n = models.load("des_s1")
    eng = make_engine(lut_graph=True, seed=1, gpu="off", **kw)
    eng.set_sbox(sbox, n)
    st = eng.initial_state()
    out = eng.create_circuit(st, eng.target(0), _core.mask_for_inputs(n))
    assert out >= 0
    st.set_output(0, out)
    assert validate_circuit(st, sbox, n, bit=0)
    return st, eng.stats()


def test_option_off_is_inert():
    st_off, stats_off = des_bit0(lut_shared=False)
    assert stats_off["candidates4s"] == 0 and stats_off["shared_hits"] == 0
    assert stats_off["scan_seconds4s"] == 0
    st_plain, _ = des_bit0()
    assert st_off.file_name() == st_plain.file_name()


def test_lut_shared_needs_lut_mode():
    with pytest.raises(ValueError):
        make_engine(lut_graph=False, lut_shared=True)


def test_cli_lut_shared_needs_lut():
    if not os.path.exists(CLI):
        pytest.skip("CLI not built (run make)")
    sbox = os.path.join(REPO, "sboxgates_amd", "sboxes", "des_s1.txt")
    proc = subprocess.run([CLI, "--lut-shared", "-o", "0", "--cpu", sbox],
                          capture_output=True, text=True, timeout=120)
    assert proc.returncode != 0
    assert "--lut-shared" in proc.stderr
    helped = subprocess.run([CLI, "--help"], capture_output=True, text=True,
                            timeout=120)
    assert "--lut-shared" in helped.stdout


# --- 5. round trip -----------------------------------------------------------

def test_shared_pair_round_trip():
    sbox, n = osh.planted_sbox(4)
    st = _core.State(4)
    o = st.add_lut(osh.PLANT_FO, 0, 1, 2)
    g = st.add_lut(osh.PLANT_FI, o, 3, 0)  # input 0 feeds both LUTs
    assert o >= 0 and g >= 0
    st.set_output(0, g)
    assert validate_circuit(st, sbox, n, bit=0)
    back = _core.State.from_xml(st.to_xml())
    assert back.fingerprint() == st.fingerprint()
    assert back.file_name() == st.file_name()
    assert back.gate(g)["in3"] == 0 and back.gate(o)["in1"] == 0
    assert validate_circuit(back, sbox, n, bit=0)
    for lang in ("hip", "cuda"):
        assert graph_to_source(st, lang)
