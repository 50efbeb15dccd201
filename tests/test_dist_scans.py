"""The distributed 5/7-LUT scan (Engine::dist_scan_chunked,
distributed_lut_body and worker_loop, driven through PyDistCtx over gloo)
against the model of the chunk protocol in _dist_model.py, on the CPU.

A scenario is one create_circuit call on a grown Rijndael pool under a sparse
two-sided mask, chosen so that steps 1-3 and the 3-LUT scan miss and exactly
one distributed node runs. Which combinations hit comes from the CPU engine's
ordered scans (hit lists, taken under two seeds); who scans what, who wins
and how many candidates every rank has looked at comes from the model. Every
assertion is an equality.

The pins below are conditions, not trusted: every check recomputes the hit
lists, and STRUCTURE names what each (launch, scenario) is there for, which
check_structure asserts of the prediction, so a pin that rots fails here
instead of testing nothing.

tests/test_gpu_dist_scans.py runs the same launches with a forced GPU on
every rank.
"""

import collections
import functools
import math

import pytest

import _dist_model as model
import _dist_scan_worker as worker
import _oracle as orc
from sboxgates_amd.ops import gen_lut_ttable, tt_eq_mask

# --- model unit tests ---------------------------------------------------------

WORLDS = range(1, 9)


def model_totals(world):
    # Divisible by the world, not divisible, prime, smaller than the world.
    return sorted({world * 12, world * 12 + 5, world * 7 + 1, 97, 5})


def model_chunks(total, world):
    longest = -(-total // world)
    shortest = total // world
    out = {0, 1, 3, 4, 5, longest, longest + 3, max(1, longest - 1)}
    if shortest:
        out.add(shortest)
    # Divisors of the shortest and the longest span.
    out.update(c for c in range(2, longest + 1)
               if longest % c == 0 or (shortest and shortest % c == 0))
    return sorted(out)


def simulate(hits, total, world, chunk):
    """The protocol played literally, candidate by candidate: (round, winner,
    hit, candidates looked at per rank), the first three None on a miss."""
    hits = set(hits)
    sp = model.spans(total, world)
    pos = [s[0] for s in sp]
    found = [None] * world
    looked = [0] * world
    longest = max(stop - start for start, stop in sp)
    c = 0
    while c == 0 or (chunk != 0 and c * chunk < longest):
        for r, (start, stop) in enumerate(sp):
            if found[r] is not None:
                continue
            end = stop if chunk == 0 else min(stop, pos[r] + chunk)
            while pos[r] < end and found[r] is None:
                if pos[r] in hits:
                    found[r] = pos[r]
                looked[r] += 1
                pos[r] += 1
        winners = [r for r in range(world) if found[r] is not None]
        if winners:
            return c, winners[0], found[winners[0]], looked
        c += 1
    return None, None, None, looked


@pytest.mark.parametrize("world", WORLDS)
def test_model_spans_partition(world):
    for total in model_totals(world):
        sp = model.spans(total, world)
        assert len(sp) == world
        assert sp[0][0] == 0 and sp[-1][1] == total
        for (_, stop), (start, _) in zip(sp, sp[1:]):
            assert stop == start
        lengths = [stop - start for start, stop in sp]
        assert min(lengths) == total // world
        assert max(lengths) == -(-total // world)


@pytest.mark.parametrize("world", WORLDS)
def test_model_rounds_cover_longest_span(world):
    for total in model_totals(world):
        longest = -(-total // world)
        for chunk in model_chunks(total, world):
            n = model.rounds(total, world, chunk)
            if chunk == 0:
                assert n == 1
            else:
                assert (n - 1) * chunk < longest <= n * chunk
            # Every rank's windows tile its span, in order, within n rounds.
            for r, (start, stop) in enumerate(model.spans(total, world)):
                at = start
                for c in range(n):
                    begin, end = model.window(total, world, chunk, r, c)
                    assert begin == at and begin <= end <= stop
                    if chunk:
                        assert end - begin <= chunk
                    at = end
                assert at == stop, (total, world, chunk, r)


def boundary_positions(total, world, chunk):
    out = set()
    for start, stop in model.spans(total, world):
        if start == stop:
            continue
        out.update((start, stop - 1))
        if chunk:
            # The last chunk of the span, short or not.
            last = start + (stop - start - 1) // chunk * chunk
            out.update((last, max(start, last - 1)))
    return sorted(out)


@pytest.mark.parametrize("world", WORLDS)
def test_model_single_hit_at_boundaries(world):
    for total in model_totals(world):
        sp = model.spans(total, world)
        for chunk in model_chunks(total, world):
            for h in boundary_positions(total, world, chunk):
                where = (total, world, chunk, h)
                p = model.predict([h], total, world, chunk)
                owner = [r for r, (a, b) in enumerate(sp) if a <= h < b]
                assert [p.winner] == owner, where
                start = sp[p.winner][0]
                assert p.round == (0 if chunk == 0 else (h - start) // chunk)
                assert p.hit == h and p.window[0] <= h < p.window[1], where
                assert p.hit_ranks == owner, where
                rnd, winner, hit, looked = simulate([h], total, world, chunk)
                assert (rnd, winner, hit) == (p.round, p.winner, p.hit), where
                assert looked == p.scanned_cpu, where
                for r in range(world):
                    lo, hi = p.scanned[r]
                    assert lo <= looked[r] <= hi, where
                    if r != winner:
                        assert lo == hi == looked[r], where


@pytest.mark.parametrize("world", WORLDS)
def test_model_against_simulation(world, rng):
    """Several hits, on several ranks and none: the prediction is what the
    literal protocol does."""
    for total in model_totals(world):
        for chunk in model_chunks(total, world)[:6]:
            for count in (0, 1, 2, 5):
                hits = sorted(rng.sample(range(total), min(count, total)))
                where = (total, world, chunk, hits)
                p = model.predict(hits, total, world, chunk)
                rnd, winner, hit, looked = simulate(hits, total, world, chunk)
                assert (rnd, winner, hit) == (p.round, p.winner, p.hit), where
                assert looked == p.scanned_cpu, where
                if not hits:
                    assert sum(looked) == total, where


# --- scenarios and launches ---------------------------------------------------

A = model.scenario(20, 24, 0)    # 5-LUT hits on all three thirds
B = model.scenario(20, 32, 2)    # no 5-LUT hit, 7-LUT hits
C = model.scenario(24, 32, 0)    # no 5-LUT hit, 7-LUT hits, larger pool
D = model.scenario(21, 27, 55)   # C(21,5) is odd; 5-LUT hits only near the end
E = model.scenario(22, 27, 55)   # C(22,5) % 4 == 2; 5-LUT hits only near the end
G = model.scenario(22, 32, 5)    # no 5-LUT hit; 7-LUT hits in the last quarter
# Pool 48, where a GPU runs the wide 5-LUT kernel, or the wave-owned one from
# set_scan5_wave_min_pool(44) on. Both nodes end with a 5-LUT hit: C(48,7) is
# too long for a hit list.
P = model.scenario(48, 26, 1)    # 5-LUT hits on the first third only
Q = model.scenario(48, 28, 1)    # 5-LUT hits on all three thirds
MAX_POOL7 = 24

Launch = collections.namedtuple("Launch",
                                "name world chunk5 chunk7 scenarios")

LAUNCHES = (
    Launch("w3", 3, 1000, 5000, (A, B, C)),
    Launch("w2", 2, 3000, 100000, (D, B)),
    Launch("w4-chunk0", 4, 0, 2000, (A, E, B)),
    Launch("w4-chunk227", 4, 227, 1000000, (G, E)),
    Launch("w3-pool48", 3, 70000, 1 << 30, (P, Q)),
)

# What each (launch, scenario) is there for; asserted by check_structure.
STRUCTURE = {
    ("w3", A): ("phase5", "winner_not_rank0", "rank0_would_hit_later",
                "several_rounds"),
    ("w3", B): ("phase7", "winner_not_rank0"),
    ("w3", C): ("phase7", "two_ranks_hit_in_final_round", "several_rounds",
                "winner_rank0"),
    ("w2", D): ("phase5", "total_not_divisible", "winner_last_rank",
                "hit_in_last_short_chunk"),
    ("w2", B): ("phase7", "chunk_larger_than_spans",
                "two_ranks_hit_in_final_round"),
    ("w4-chunk0", A): ("phase5", "one_round", "two_ranks_hit_in_final_round",
                       "winner_rank0"),
    ("w4-chunk0", E): ("phase5", "one_round", "total_not_divisible",
                       "winner_last_rank"),
    ("w4-chunk0", B): ("phase7", "several_rounds", "winner_not_rank0"),
    ("w4-chunk227", G): ("phase7", "chunk_larger_than_spans",
                         "total5_not_divisible", "last_round_of_one_candidate",
                         "winner_last_rank"),
    ("w4-chunk227", E): ("phase5", "several_rounds", "total_not_divisible",
                         "winner_last_rank"),
    ("w3-pool48", P): ("phase5", "several_rounds", "winner_rank0"),
    ("w3-pool48", Q): ("phase5", "winner_last_rank", "rank0_would_hit_later"),
}


@functools.lru_cache(maxsize=None)
def scenario_reference(scen):
    """(state, target, mask, 5-LUT hit list, 7-LUT hit list or None) of a
    scenario; the 7-LUT list only where no 5-LUT hit ends the node first.
    Asserts that no 3-LUT hits. Computed once and shared; nobody changes it."""
    eng = orc.cpu_engine(5)
    st, target, mask = model.scenario_setup(eng, scen)
    n = st.num_gates
    for seed in model.HIT_SEEDS:
        found, _, evaluated = eng.scan_pool(3, st, target, mask, 0,
                                            math.comb(n, 3), seed=seed)
        assert not found and evaluated == math.comb(n, 3), scen
    hits5 = model.hit_list(eng, 5, st, target, mask)
    assert hits5 or n <= MAX_POOL7, (scen, "no 5-LUT hit")
    hits7 = None if hits5 else model.hit_list(eng, 7, st, target, mask)
    return st, target, mask, tuple(hits5), hits7 and tuple(hits7)


def predict_node(scen, launch):
    """(phase k, Prediction of the 5-LUT scan, Prediction of the 7-LUT scan
    or None, hit list of phase k)."""
    st, _, _, hits5, hits7 = scenario_reference(scen)
    n = st.num_gates
    p5 = model.predict(hits5, math.comb(n, 5), launch.world, launch.chunk5)
    if p5.winner is not None:
        return 5, p5, None, hits5
    assert not hits5, "no 5-LUT hit"
    p7 = model.predict(hits7, math.comb(n, 7), launch.world, launch.chunk7)
    assert p7.winner is not None, "the node must end with a 7-LUT hit"
    return 7, p5, p7, hits7


def check_structure(scen, launch):
    k, p5, p7, hits = predict_node(scen, launch)
    n = scen[0]
    p = p5 if k == 5 else p7
    chunk = launch.chunk5 if k == 5 else launch.chunk7
    total = math.comb(n, k)
    W = launch.world
    facts = {
        "phase5": k == 5,
        "phase7": k == 7,
        "winner_not_rank0": p.winner != 0,
        "winner_rank0": p.winner == 0,
        "winner_last_rank": p.winner == W - 1,
        "rank0_would_hit_later": k == 5 and p.winner != 0 and any(
            h < model.spans(total, W)[0][1] for h in hits),
        "several_rounds": p.round >= 1,
        "one_round": model.rounds(total, W, chunk) == 1,
        "two_ranks_hit_in_final_round": len(p.hit_ranks) >= 2,
        "total_not_divisible": total % W != 0,
        "total5_not_divisible": math.comb(n, 5) % W != 0,
        "chunk_larger_than_spans": chunk > -(-total // W),
        "hit_in_last_short_chunk": (
            chunk != 0 and p.round == model.rounds(total, W, chunk) - 1
            and p.window[1] - p.window[0] < chunk
            and all(h >= p.window[0] for h in hits)),
        # floor(total / W) is a multiple of the 5-LUT chunk and total is not
        # a multiple of W: the last round holds one candidate of the longer
        # spans, and a round count taken from the rounded-down span loses it.
        "last_round_of_one_candidate": (
            launch.chunk5 != 0 and math.comb(n, 5) % W != 0
            and (math.comb(n, 5) // W) % launch.chunk5 == 0),
    }
    for name in STRUCTURE[launch.name, scen]:
        assert facts[name], (launch.name, scen, name)


def expected_scans(total, world, chunk, last):
    """Per rank: the number of non-empty windows through round `last`."""
    out = []
    for r in range(world):
        windows = [model.window(total, world, chunk, r, c)
                   for c in range(last + 1)]
        out.append(sum(1 for begin, end in windows if begin < end))
    return out


def check_scenario(results, launch, idx, mode):
    """results[rank][idx] of one launch against the model. mode is "cpu",
    "gpu-ordered" or "gpu-default"."""
    scen = launch.scenarios[idx]
    where = (launch.name, scen, mode)
    check_structure(scen, launch)
    st, target, mask, _, _ = scenario_reference(scen)
    n = st.num_gates
    W = launch.world
    k, p5, p7, hits = predict_node(scen, launch)
    p = p5 if k == 5 else p7
    recs = [results[r][idx] for r in range(W)]
    stats = [rec["stats"] for rec in recs]

    # Exactly one node, whose 3-LUT scan missed over all of C(n, 3): steps
    # 1-3 added nothing, and no recursion followed.
    assert stats[0]["nodes"] == 1, where
    assert stats[0]["candidates3"] == math.comb(n, 3), where
    for r in range(1, W):
        assert stats[r]["nodes"] == 0 and stats[r]["candidates3"] == 0, where

    # The phase that ended the node, and what it added.
    rec = recs[0]
    added = rec["added"]
    assert rec["pool"] == n, where
    assert len(added) == (2 if k == 5 else 3), (where, added)
    assert all(g["type_name"] == "LUT" for g in added), (where, added)
    assert rec["returned"] == n + len(added) - 1, where
    inputs = [g[key] for g in added for key in ("in1", "in2", "in3")]
    pool_ids = sorted(i for i in inputs if i < n)
    assert len(pool_ids) == k == len(set(pool_ids)), (where, added)
    assert sorted(i for i in inputs if i >= n) == list(
        range(n, n + len(added) - 1)), (where, added)
    got = orc.checked_rank(pool_ids, n)
    if mode == "gpu-default":
        assert got in hits and p.window[0] <= got < p.window[1], (
            where, got, p.window)
    else:
        assert got == p.hit, (where, got, p.hit, pool_ids)
        assert pool_ids == orc.checked_unrank(p.hit, n, k), where

    # The returned gate, rebuilt from the added LUTs' inputs and functions.
    tabs = {i: st.gate(i)["table"] for i in range(n)}
    for j, g in enumerate(added):
        assert 0 < g["function"] < 256, (where, g)
        tabs[n + j] = gen_lut_ttable(g["function"], tabs[g["in1"]],
                                     tabs[g["in2"]], tabs[g["in3"]])
    assert rec["table"] == tabs[rec["returned"]].hex(), where
    assert tt_eq_mask(target, tabs[rec["returned"]], mask), where

    # Candidates per rank and kind.
    for kind, pk, chunk in ((5, p5, launch.chunk5), (7, p7, launch.chunk7)):
        counts = [s["candidates%d" % kind] for s in stats]
        if pk is None:
            assert counts == [0] * W, (where, kind, counts)
            continue
        for r in range(W):
            lo, hi = pk.scanned[r]
            if mode == "cpu":
                assert counts[r] == pk.scanned_cpu[r], (where, kind, r, counts)
            elif mode == "gpu-ordered" or lo == hi:
                assert lo <= counts[r] <= hi, (where, kind, r, counts)
            else:
                # Default election: the windows before the final one missed
                # and count whole; of the final one nothing is promised but
                # that no more than the window was looked at.
                assert lo - 1 <= counts[r] <= hi, (where, kind, r, counts)
        if pk.winner is None:
            assert sum(counts) == math.comb(n, kind), (where, kind, counts)

    # Scans per rank: one per non-empty window, and rank 0's 3-LUT scan.
    scans = [1] + [0] * (W - 1)
    for kind, pk, chunk in ((5, p5, launch.chunk5), (7, p7, launch.chunk7)):
        if pk is None:
            continue
        total = math.comb(n, kind)
        last = (pk.round if pk.winner is not None
                else model.rounds(total, W, chunk) - 1)
        for r, v in enumerate(expected_scans(total, W, chunk, last)):
            scans[r] += v
    on, off = (("cpu_scans", "gpu_scans") if mode == "cpu"
               else ("gpu_scans", "cpu_scans"))
    assert [s[on] for s in stats] == scans, (where, stats)
    assert [s[off] for s in stats] == [0] * W, (where, stats)
    assert all(v > 0 for v in scans), where


def run_launch(launch, tmp_path, gpu="off", ordered=False, wave_min_pool=None):
    job = {"mode": "scenarios", "gpu": gpu, "ordered": ordered,
           "wave_min_pool": wave_min_pool,
           "scenarios": [list(s) for s in launch.scenarios]}
    results = worker.launch(job, launch.world, tmp_path, chunk5=launch.chunk5,
                            chunk7=launch.chunk7)
    assert sorted(results) == list(range(launch.world))
    for r in results:
        assert len(results[r]) == len(launch.scenarios)
    return results


@pytest.fixture(scope="module")
def cpu_launch(tmp_path_factory):
    """launch -> its results on the CPU; every launch runs once."""
    @functools.lru_cache(maxsize=None)
    def run(launch):
        return run_launch(launch, tmp_path_factory.mktemp(launch.name))
    return run


@pytest.mark.parametrize("launch", LAUNCHES, ids=lambda l: l.name)
def test_scenarios_match_model(launch, cpu_launch):
    results = cpu_launch(launch)
    for idx in range(len(launch.scenarios)):
        check_scenario(results, launch, idx, "cpu")


def test_pinned_counts(cpu_launch):
    """The three starting pins, as recorded when they were chosen: the model
    and the engine have to agree on these figures, not only on each other."""
    launch = LAUNCHES[0]
    assert (launch.world, launch.chunk5, launch.chunk7) == (3, 1000, 5000)
    assert scenario_reference(A)[3] == (3265, 6407, 8723)
    assert scenario_reference(B)[3] == () and scenario_reference(B)[4][0] == 27497
    assert scenario_reference(C)[3] == () and scenario_reference(C)[4][0] == 15586
    k, p5, _, _ = predict_node(A, launch)
    assert (k, p5.round, p5.winner, p5.hit) == (5, 1, 1, 6407)
    assert p5.scanned_cpu == [2000, 1240, 2000]
    k, p5, p7, _ = predict_node(B, launch)
    assert k == 7 and p5.scanned_cpu == [5168] * 3
    assert sum(p5.scanned_cpu) == math.comb(20, 5)
    assert (p7.round, p7.winner) == (0, 1)
    k, p5, p7, _ = predict_node(C, launch)
    assert (k, p7.round, p7.winner, p7.hit) == (7, 3, 0, 15586)
    assert p7.hit_ranks == [0, 1] and p7.scanned_cpu[2] == 20000
    results = cpu_launch(launch)
    assert [results[r][0]["stats"]["candidates5"] for r in range(3)] == [
        2000, 1240, 2000]
    assert [results[r][1]["stats"]["candidates5"] for r in range(3)] == [
        5168] * 3
    assert results[2][2]["stats"]["candidates7"] == 20000


# --- a whole search -----------------------------------------------------------

SEARCH_WORLD = 3
SEARCH_CHUNKS = (500, 5000)


def run_search(tmp_path, gpu, seed=21):
    job = {"mode": "search", "gpu": gpu, "ordered": True, "seed": seed}
    tmp_path.mkdir(exist_ok=True)
    results = worker.launch(job, SEARCH_WORLD, tmp_path,
                            chunk5=SEARCH_CHUNKS[0], chunk7=SEARCH_CHUNKS[1])
    # Many rounds: every rank scanned 5-LUT and 7-LUT windows.
    for r in range(SEARCH_WORLD):
        stats = results[r]["stats"]
        assert stats["candidates5"] > 0 and stats["candidates7"] > 0, (r, stats)
    return results


def test_ordered_search_reproducible(tmp_path):
    """DES S1 bit 0, LUT mode, seeded, ordered, three ranks, many rounds: two
    gpu="off" runs write the same circuit, byte for byte, and scan the same
    number of candidates on every rank. (Not compared with the one-rank
    search, which is documented to differ.)"""
    first = run_search(tmp_path / "a", "off")
    again = run_search(tmp_path / "b", "off")
    assert first[0]["xml"] == again[0]["xml"]
    assert first[0]["file_name"] == again[0]["file_name"]
    for r in range(SEARCH_WORLD):
        assert first[r]["stats"] == again[r]["stats"], r
