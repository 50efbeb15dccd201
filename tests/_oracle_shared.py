"""Independent reference for the shared-input two-LUT scan, shared by the
CPU and GPU tests of it: pure Python and numpy, written from the scan's
definition. Like tests/_oracle.py, whose helpers it imports, it uses none of
the engine's cell algebra; hits are re-evaluated with _oracle.hit_table(5,
...), since the result layout is the 5-LUT one.

A 4-combination g0 < g1 < g2 < g3 hits when, for some rest gate d among the
four and some shared gate s among the other three (x, y, z, ascending),
LUT(fi; LUT(fo; x, y, z), d, s) realises the target under the mask.
"""

import functools
import math

import numpy as np

import _oracle as orc
from sboxgates_amd import _core
from sboxgates_amd.ops import make_engine, scan_shared
from sboxgates_amd.utils import validate_circuit

_FO = np.arange(256, dtype=np.int64)

# Outer and inner function of the planted shape: f(a, b, c, d) =
# a ? ((b ^ c) & d) : ((b & c) ^ d) as LUT(FI; LUT(FO; a, b, c), d, a).
PLANT_FO = sum(1 << (a << 2 | b << 1 | c)
               for a in (0, 1) for b in (0, 1) for c in (0, 1)
               if ((b ^ c) if a else (b & c)))
PLANT_FI = sum(1 << (o << 2 | d << 1 | s)
               for o in (0, 1) for d in (0, 1) for s in (0, 1)
               if ((o & d) if s else (o ^ d)))


def planted_f(a, b, c, d):
    return ((b ^ c) & d) if a else ((b & c) ^ d)


def planted_sbox(num_inputs):
    """One-output S-box of f over inputs 0..3; further inputs are ignored."""
    table = [planted_f(x & 1, (x >> 1) & 1, (x >> 2) & 1, (x >> 3) & 1)
             for x in range(1 << num_inputs)]
    return _core.load_sbox_table(table)


def planted_search(num_inputs, seed, gpu="off", **kw):
    """(LUTs added, stats) of create_circuit on bit 0 of the planted S-box."""
    sbox, n = planted_sbox(num_inputs)
    assert n == num_inputs
    eng = make_engine(lut_graph=True, seed=seed, gpu=gpu, **kw)
    eng.set_sbox(sbox, n)
    st = eng.initial_state()
    out = eng.create_circuit(st, eng.target(0), _core.mask_for_inputs(n))
    assert out >= 0
    st.set_output(0, out)
    assert validate_circuit(st, sbox, n, bit=0)
    return st.num_gates - n, eng.stats()


def shape_positions(shape):
    """(outer triple positions, rest position, shared position) of a shape
    number 3 * r + si inside the ascending 4-combination."""
    r, si = divmod(shape, 3)
    triple = [j for j in range(4) if j != r]
    return triple, r, triple[si]


def found4s(tabs, target, mask):
    """Shared-input verdict: some rest gate, some shared gate and some outer
    function among all 256 leave no inner cell (o, d, s) with both target-1
    and target-0 content."""
    pos = orc.positions(mask)
    tgt = [(target >> p) & 1 for p in pos]
    for r in range(4):
        triple = [j for j in range(4) if j != r]
        po = orc.patterns([tabs[j] for j in triple], pos)
        pd = [(tabs[r] >> p) & 1 for p in pos]
        for sj in triple:
            ps = [(tabs[sj] >> p) & 1 for p in pos]
            # Per inner pattern v = (d, s): the outer patterns seen with
            # target 1 / 0.
            a1 = [0] * 4
            a0 = [0] * 4
            for u, d, s, t in zip(po, pd, ps, tgt):
                if t:
                    a1[d << 1 | s] |= 1 << u
                else:
                    a0[d << 1 | s] |= 1 << u
            bad = np.zeros(256, dtype=bool)
            for v in range(4):
                bad |= ((_FO & a1[v]) != 0) & ((_FO & a0[v]) != 0)
                bad |= ((~_FO & a1[v]) != 0) & ((~_FO & a0[v]) != 0)
            if not bad.all():
                return True
    return False


def has_3lut_subset(tabs, target, mask):
    """True if some three of the four gates already admit one 3-LUT."""
    return any(orc.found3([tabs[j] for j in range(4) if j != r], target, mask)
               for r in range(4))


def assert_hit_layout(res, comb):
    """A hit names exactly the combination, in the 5-LUT layout with the
    shared gate repeated."""
    assert sorted(set(res[2:7])) == list(comb), (res, comb)
    assert list(res[2:5]) == sorted(res[2:5]), res
    assert res[6] in res[2:5], res
    assert res[5] not in res[2:5], res


# (pool, mask size) of the per-rank cases: single-rank windows over all of
# C(pool, 4), Rijndael bit-0 target, pool grown with POOL_SEED + pool.
SHARED_CASES = [(12, 8), (12, 10), (16, 8), (16, 10)]
EXCL = 0b10100101


def case_id(case):
    return "pool%d-mask%d" % case


@functools.lru_cache(maxsize=None)
def case_setup(case):
    """(state, target, mask, total ranks) of a per-rank case."""
    pool, size = case
    eng = orc.cpu_engine(5)
    st = eng.initial_state()
    st.grow_pool_random(pool, orc.POOL_SEED + pool)
    assert st.num_gates == pool
    target = eng.target(0)
    mask = orc.sparse_mask(6000 + 10 * pool + size, size, target)
    return st, target, mask, math.comb(pool, 4)


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """Per rank: (combination, oracle verdict, a 3-subset is 3-LUT-feasible,
    CPU found, CPU res). Computed once and shared."""
    pool, _ = case
    st, target, mask, total = case_setup(case)
    eng = orc.cpu_engine(5)
    tabs = [orc.tt_int(st.gate(i)["table"]) for i in range(pool)]
    t, m = orc.tt_int(target), orc.tt_int(mask)
    out = []
    for r in range(total):
        comb = orc.checked_unrank(r, pool, 4)
        g = [tabs[i] for i in comb]
        f_c, r_c, ev = scan_shared(eng, st, target, mask, r, r + 1,
                                   seed=orc.SCAN_SEED)
        assert ev == 1, (case, r)
        out.append((comb, found4s(g, t, m), has_3lut_subset(g, t, m), f_c,
                    tuple(r_c)))
    return tuple(out)
