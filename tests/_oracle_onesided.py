"""The per-rank cases on one-sided masks (_oracle.onesided_masks), shared
by the CPU tests of tests/test_oracle.py and the GPU tests of
tests/test_gpu_onesided_masks.py: the CPU scan of every single-rank window,
computed once per (kind, mask) and never changed.

Kinds: 3, 4, 5 and 7 are the scans of scan_pool; "s" is the shared-input
scan, whose results have the 5-LUT layout. Target: Rijndael bit 0; pools
grown with POOL_SEED + pool, as for the other per-rank cases.
"""

import functools
import math

import _oracle as orc

# kind -> pool
POOLS = {3: 24, 4: 24, 5: 12, "s": 16, 7: 10}
KINDS = tuple(POOLS)
MASK_SEED = 0x0517
# The masks under which a scan has to give both answers, for these kinds.
TWO_SIDED = ("Zall", "Z40")
TWO_SIDED_KINDS = (3, 4, 5, "s")


def kind_id(kind):
    return "shared" if kind == "s" else "k%d" % kind


def width(kind):
    """Gates of a combination."""
    return {3: 3, 4: 3, 5: 5, "s": 4, 7: 7}[kind]


def layout(kind):
    """The k of _oracle.hit_table for the kind's result layout."""
    return 5 if kind == "s" else kind


def engine_kind(kind):
    """The k of _oracle.cpu_engine for an engine that runs the kind."""
    return 4 if kind == 4 else 3


def scan(eng, kind, st, target, mask, begin, end, **kw):
    if kind == "s":
        return eng.scan_shared(st, target, mask, begin, end, **kw)
    return eng.scan_pool(kind, st, target, mask, begin, end, **kw)


def hit_ids(kind, res):
    if kind == "s":
        return sorted(set(res[2:7]))
    return orc.hit_ids(kind, res)


@functools.lru_cache(maxsize=None)
def setup(kind, pool=None):
    """(state, target, {name: mask}, total ranks) of a kind."""
    pool = pool or POOLS[kind]
    eng = orc.cpu_engine(engine_kind(kind))
    st = eng.initial_state()
    st.grow_pool_random(pool, orc.POOL_SEED + pool)
    assert st.num_gates == pool
    target = eng.target(0)
    return (st, target, orc.onesided_masks(target, MASK_SEED),
            math.comb(pool, width(kind)))


@functools.lru_cache(maxsize=None)
def reference(kind, name):
    """Per rank: (combination, CPU found, CPU res, CPU evaluated)."""
    st, target, masks, total = setup(kind)
    eng = orc.cpu_engine(engine_kind(kind))
    out = []
    for r in range(total):
        f_c, r_c, ev_c = scan(eng, kind, st, target, masks[name], r, r + 1,
                              seed=orc.SCAN_SEED)
        out.append((orc.checked_unrank(r, POOLS[kind], width(kind)), bool(f_c),
                    tuple(r_c), ev_c))
    return tuple(out)


def hit_ranks(kind, name):
    return [r for r, row in enumerate(reference(kind, name)) if row[1]]


FIRST_HITS = 8


def ordered_windows(kind, name):
    """Windows of the ordered engine: the whole space, and from one past
    each of the first eight CPU hits to its end."""
    total = setup(kind)[3]
    return [(0, total)] + [(h + 1, total)
                           for h in hit_ranks(kind, name)[:FIRST_HITS]
                           if h + 1 < total]


def check_hit(kind, st, comb, res, target, mask):
    """A hit names the rank's combination, realises the target under the
    mask and holds no zero function byte."""
    threes = orc.threes_default() if kind == 4 else None
    assert hit_ids(kind, res) == list(comb), (kind, comb, list(res))
    orc.assert_hit_valid(layout(kind), st, res, target, mask, threes)
    orc.assert_no_zero_function(layout(kind), res, threes)
