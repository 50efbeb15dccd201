"""A model of the chunked distributed scan, written from its definition and
not from the engine: who scans which ranks of C(n, k) in which round, who
wins, and how many candidates every rank has looked at when the scan ends.

For a space of `total` ranks, world W and chunk size `chunk`:

* rank r owns [total*r//W, total*(r+1)//W);
* every rank runs ceil(ceil(total/W)/chunk) rounds, one if chunk == 0;
* in round c a rank that has not hit yet scans the next `chunk` ranks of its
  span, clipped to the span (its whole span if chunk == 0);
* after every round the lowest rank id that has hit so far wins and the scan
  ends; with no winner after the last round the scan misses.

Whether a combination hits is taken from the CPU engine's ordered scan
(hit_list), which tests/test_oracle.py holds to an independent oracle per
candidate. The distributed search draws its own scan seed, so hit_list takes
the list under two seeds and insists that they agree: the model holds where
verdicts do not depend on the seed, which two-sided masks guarantee
(docs/PARITY.md, "One-sided masks").
"""

import bisect
import collections
import math

import _oracle as orc

HIT_SEEDS = (7, 8)


def spans(total, world):
    return [(total * r // world, total * (r + 1) // world)
            for r in range(world)]


def rounds(total, world, chunk):
    longest = -(-total // world)
    return 1 if chunk == 0 else -(-longest // chunk)


def window(total, world, chunk, r, c):
    """[begin, end) that rank r scans in round c, had it not hit before;
    empty once its span is used up."""
    start, stop = spans(total, world)[r]
    if chunk == 0:
        return (start, stop) if c == 0 else (stop, stop)
    return min(stop, start + c * chunk), min(stop, start + (c + 1) * chunk)


Prediction = collections.namedtuple(
    "Prediction", "round winner window hit scanned scanned_cpu hit_ranks")
Prediction.__doc__ = """What a distributed scan does. round, winner, window
and hit are None on a miss; otherwise the winning round, the winner's rank
id, its window in that round and the lowest hit in that window. scanned[r]
is the interval (lo, hi) of the number of candidates rank r evaluated, lo ==
hi for a rank that never hit; scanned_cpu[r] is the exact count where a scan
that hits at offset o of its window counts o + 1, as the CPU scans do.
hit_ranks are the ranks that hit in the final round."""


def predict(hits, total, world, chunk):
    hits = sorted(hits)
    assert not hits or 0 <= hits[0] and hits[-1] < total
    sp = spans(total, world)
    nrounds = rounds(total, world, chunk)
    # Per rank: its first hit and the round that finds it.
    first = []
    for r, (start, stop) in enumerate(sp):
        i = bisect.bisect_left(hits, start)
        if i < len(hits) and hits[i] < stop:
            h = hits[i]
            first.append((h, 0 if chunk == 0 else (h - start) // chunk))
        else:
            first.append(None)
    hit_rounds = [f[1] for f in first if f is not None]
    if hit_rounds:
        last = min(hit_rounds)
        assert last < nrounds
    else:
        last = nrounds - 1
    hit_ranks = [r for r, f in enumerate(first)
                 if f is not None and f[1] == last]
    scanned, scanned_cpu = [], []
    for r, (start, stop) in enumerate(sp):
        begin, end = window(total, world, chunk, r, last)
        if r in hit_ranks:
            before = begin - start
            scanned.append((before + 1, end - start))
            scanned_cpu.append(before + first[r][0] - begin + 1)
        else:
            scanned.append((end - start, end - start))
            scanned_cpu.append(end - start)
    if not hit_ranks:
        return Prediction(None, None, None, None, scanned, scanned_cpu, [])
    winner = hit_ranks[0]
    win = window(total, world, chunk, winner, last)
    assert win[0] <= first[winner][0] < win[1]
    return Prediction(last, winner, win, first[winner][0], scanned,
                      scanned_cpu, hit_ranks)


def hit_list_seeded(engine, k, st, target, mask, seed):
    n = st.num_gates
    total = math.comb(n, k)
    hits = []
    begin = 0
    while begin < total:
        found, res, _ = engine.scan_pool(k, st, target, mask, begin, total,
                                         seed=seed)
        if not found:
            break
        orc.assert_hit_valid(k, st, res, target, mask)
        r = orc.checked_rank(orc.hit_ids(k, res), n)
        assert begin <= r < total, (k, begin, r)
        hits.append(r)
        begin = r + 1
    return hits


def hit_list(engine, k, st, target, mask):
    """Every hitting rank of C(n, k), ascending, from the CPU engine's
    ordered scan restarted behind each hit; the same under both HIT_SEEDS."""
    orc.assert_mask_has_target1(target, mask)
    assert orc.tt_int(mask) & ~orc.tt_int(target), "mask is one-sided"
    lists = [hit_list_seeded(engine, k, st, target, mask, s)
             for s in HIT_SEEDS]
    assert lists[0] == lists[1], (k, "verdicts depend on the scan seed")
    return lists[0]


# --- scenarios ----------------------------------------------------------------

POOL_SEED = 0xA1


def scenario(n, size, i, bit=0, pool_seed=POOL_SEED):
    """(pool size, pool seed, S-box bit, mask seed, mask size)."""
    return (n, pool_seed, bit, 100 * size + i, size)


def scenario_setup(engine, scen):
    """(state, target, mask) of a scenario on a Rijndael engine: the initial
    state grown to n gates, one output bit, a seeded two-sided sparse mask."""
    n, pool_seed, bit, mask_seed, size = scen
    st = engine.initial_state()
    st.grow_pool_random(n, pool_seed)
    assert st.num_gates == n
    target = engine.target(bit)
    return st, target, orc.sparse_mask(mask_seed, size, target)
