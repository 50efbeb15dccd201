"""GPU scans on masks that hold no target-1 position, no target-0 position
or no position at all (_oracle.onesided_masks). create_circuit halves its
mask at every level and has no special case for such masks, so deep nodes
issue them. On them no cell is live, every candidate passes the screens and
goes down the survivor path (in k_scan5_wave the on-demand prefix-cell
build), and the verdict rests on the "function 00 does not round-trip"
rules of sbg/lutcover.hpp.

Every expectation is the CPU scan's of the same window and seed
(_oracle_onesided.reference, which tests/test_oracle.py checks on its own),
the k=3 rule _oracle.found3_onesided, the pair oracle of _oracle_pairs.py, or
the re-evaluation of the hit; none comes from a GPU run.

CPU hits per rank, Rijndael bit 0 (the other masks hit on every rank):
k=3 pool 24: Zall 1089, Z40 1315 of 2024; k=4 pool 24: Zall 1089, Z40 1315,
O40 1415, Oall 1099 of 2024; k=5 pool 12: Zall 645, Z40 736 of 792; shared
pool 16: Zall 1568, Z40 1751 of 1820; k=7 pool 10: all 120 under every mask.
"""

import pytest

import _oracle as orc
import _oracle_onesided as one
import _oracle_pairs as op
from sboxgates_amd import _core, models
from sboxgates_amd.ops import make_engine, mask_for_inputs, tt_eq_mask
from test_scan5_aligned import aes_target, pool as pool5

pytestmark = pytest.mark.gpu

LUT_KINDS = (3, 5, "s", 7)
PATHS = ("service", "oneshot")


def need_gpu():
    if not _core.gpu_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def lut_gpu():
    need_gpu()
    gpu = orc.rijndael_engine(True, gpu="force")
    assert gpu.gpu_active
    return gpu


@pytest.fixture(scope="module")
def lut_ordered():
    need_gpu()
    gpu = orc.rijndael_engine(True, gpu="force", ordered=True)
    assert gpu.gpu_active
    return gpu


def k4_gpu(monkeypatch, path, **kw):
    """A fresh k=4 engine; it decides between the scan service and the
    one-shot kernel on its first scan, from the environment as it is then."""
    need_gpu()
    if path == "service":
        monkeypatch.delenv("SBOXGATES_NO_SVC", raising=False)
    else:
        monkeypatch.setenv("SBOXGATES_NO_SVC", "1")
    gpu = orc.rijndael_engine(False, gpu="force", try_nots=True, **kw)
    assert gpu.gpu_active
    return gpu


def check_ran_on_gpu(gpu, scans, before=0):
    stats = gpu.stats()
    assert stats["cpu_scans"] == 0, stats
    assert stats["gpu_scans"] - before == scans, (stats, before, scans)


# --- 1. per rank ------------------------------------------------------------

def check_per_rank(gpu, kind, name):
    """Every single-rank window of the kind under mask `name`; returns the
    number of scans."""
    st, target, masks, total = one.setup(kind)
    mask = masks[name]
    ref = one.reference(kind, name)
    assert len(ref) == total
    tabs = [orc.tt_int(st.gate(i)["table"]) for i in range(st.num_gates)]
    t, m = orc.tt_int(target), orc.tt_int(mask)
    for r, (comb, f_c, r_c, ev_c) in enumerate(ref):
        f_g, r_g, ev_g = one.scan(gpu, kind, st, target, mask, r, r + 1,
                                  seed=orc.SCAN_SEED)
        where = (one.kind_id(kind), name, r, comb)
        assert bool(f_g) == f_c, where
        assert ev_g == ev_c == 1, where
        if kind == 3:
            assert f_g == orc.found3_onesided([tabs[i] for i in comb], t, m), \
                where
        if not f_g:
            continue
        one.check_hit(kind, st, comb, r_g, target, mask)
        if kind != 7:
            # No election in a single-candidate window: the CPU's words. The
            # k=7 winner among orderings is a race.
            assert tuple(r_g) == r_c, (where, list(r_g), list(r_c))
    return total


@pytest.mark.parametrize("name", orc.ONESIDED)
@pytest.mark.parametrize("kind", LUT_KINDS, ids=one.kind_id)
def test_lut_scans_per_rank(lut_gpu, kind, name):
    before = lut_gpu.stats()["gpu_scans"]
    scans = check_per_rank(lut_gpu, kind, name)
    check_ran_on_gpu(lut_gpu, scans, before)


@pytest.mark.parametrize("name", orc.ONESIDED)
@pytest.mark.parametrize("path", PATHS)
def test_scan4_per_rank(monkeypatch, capfd, path, name):
    gpu = k4_gpu(monkeypatch, path)
    scans = check_per_rank(gpu, 4, name)
    check_ran_on_gpu(gpu, scans)
    # A service that fails hands its engine to the one-shot kernel and says
    # so; that must not be how this test passed.
    assert "scan service disabled" not in capfd.readouterr().err


def pair_engine(monkeypatch, path):
    need_gpu()
    if path == "service":
        monkeypatch.delenv("SBOXGATES_NO_SVC", raising=False)
    else:
        monkeypatch.setenv("SBOXGATES_NO_SVC", "1")
    gpu = op.rijndael_engine(gpu="force")
    assert gpu.gpu_active
    return gpu


def check_pairs_per_rank(gpu, name):
    """k=2 at pool 24, both function lists, identity and shuffled order;
    returns the number of scans."""
    cpu = op.cpu_engine()
    st, target, _ = op.case_setup(op.MASK_SIZES[0])
    mask = orc.onesided_masks(target, one.MASK_SEED)[name]
    tabs = [orc.tt_int(st.gate(i)["table"]) for i in range(op.POOL)]
    t = orc.tt_int(target)
    pos = orc.positions(orc.tt_int(mask))
    scans = 0
    for which in op.LISTS:
        funs = op.fun_lists()[which]
        for order_name in ("identity", "shuffled"):
            order = op.orders(op.POOL)[order_name]
            arg = None if order_name == "identity" else order
            for r in range(op.TOTAL):
                got = gpu.scan_pairs(st, target, mask, r, r + 1, which, arg)
                ref = cpu.scan_pairs(st, target, mask, r, r + 1, which, arg)
                scans += 1
                where = (name, which, order_name, r)
                assert (got[0], list(got[1]), got[2]) == (
                    ref[0], list(ref[1]), ref[2]), where
                assert got[2] == 1, where
                i, k = op.pair_of_rank(r, op.POOL)
                verdict = op.pair_verdict(tabs[order[i]], tabs[order[k]], t,
                                          pos, funs)
                assert got[0] == (verdict is not None), where
                if got[0]:
                    assert tuple(got[1][:4]) == op.expected(
                        verdict, order[i], order[k]), where
                    op.assert_hit_valid(st, funs, got[1], target, mask)
    return scans


@pytest.mark.parametrize("name", orc.ONESIDED)
@pytest.mark.parametrize("path", PATHS)
def test_pair_scan_per_rank(monkeypatch, capfd, path, name):
    gpu = pair_engine(monkeypatch, path)
    scans = check_pairs_per_rank(gpu, name)
    stats = gpu.stats()
    assert stats["pair_scans_gpu"] == scans and stats["pair_scans_cpu"] == 0
    assert stats["cpu_scans"] == 0
    assert "scan service disabled" not in capfd.readouterr().err


# --- 2. the ordered engine --------------------------------------------------

def check_ordered(gpu, kind, name):
    """Returns the number of scans."""
    st, target, masks, total = one.setup(kind)
    mask = masks[name]
    cpu = orc.cpu_engine(one.engine_kind(kind))
    hits = one.hit_ranks(kind, name)
    windows = one.ordered_windows(kind, name)
    assert len(windows) == one.FIRST_HITS + 1
    for begin, end in windows:
        where = (one.kind_id(kind), name, begin, end)
        f_c, r_c, ev_c = one.scan(cpu, kind, st, target, mask, begin, end,
                                  seed=orc.SCAN_SEED)
        inside = [h for h in hits if begin <= h < end]
        assert bool(f_c) == bool(inside), where
        # Raises "hits on the GPU and misses on the CPU" where the two
        # disagree on the lowest rank.
        f_g, r_g, ev_g = one.scan(gpu, kind, st, target, mask, begin, end,
                                  seed=orc.SCAN_SEED)
        assert bool(f_g) == bool(f_c), where
        if not f_c:
            assert ev_g == ev_c == end - begin, where
            continue
        assert list(r_g) == list(r_c), (where, list(r_g), list(r_c))
        assert 1 <= ev_g <= end - begin, where
        one.check_hit(kind, st, one.reference(kind, name)[inside[0]][0], r_g,
                      target, mask)
    return len(windows)


@pytest.mark.parametrize("name", orc.ONESIDED)
@pytest.mark.parametrize("kind", LUT_KINDS, ids=one.kind_id)
def test_lut_scans_ordered(lut_ordered, kind, name):
    before = lut_ordered.stats()["gpu_scans"]
    scans = check_ordered(lut_ordered, kind, name)
    check_ran_on_gpu(lut_ordered, scans, before)


@pytest.mark.parametrize("name", orc.ONESIDED)
@pytest.mark.parametrize("path", PATHS)
def test_scan4_ordered(monkeypatch, capfd, path, name):
    gpu = k4_gpu(monkeypatch, path, ordered=True)
    scans = check_ordered(gpu, 4, name)
    check_ran_on_gpu(gpu, scans)
    assert "scan service disabled" not in capfd.readouterr().err


# --- 3. the wide and the wave 5-LUT kernels ---------------------------------

WIDE_POOLS = (65, 100)
WIDE_MASKS = ("Zall", "Z40", "O40", "E")
WAVES_PER_BLOCK = 4
FOLLOW_UPS = 3


def triple_span(n, triple):
    c = triple[2]
    return (orc.checked_rank(triple + (c + 1, c + 2), n),
            orc.checked_rank(triple + (n - 2, n - 1), n) + 1)


def wide_windows(n):
    """(begin, end, what) of the windows: all pairs of a triple with a long
    row; 16 consecutive triples, which the wave kernel takes in more than
    one chunk; the pool's last triple."""
    assert n - 1 - 20 > _core.SCAN5_WIDE_MIN_ROW
    run = [(0, 1, c) for c in range(5, 21)]
    units = len(run)
    # The grid of the host: a wave per SCAN5_CHUNK_MIN triples.
    waves = WAVES_PER_BLOCK * min(
        2048, units // (WAVES_PER_BLOCK * _core.SCAN5_CHUNK_MIN) + 1)
    chunks = _core.scan5_chunks(units, waves)
    assert len(chunks) >= 2 and sum(c for _, c in chunks) == units, chunks
    last = (n - 5, n - 4, n - 3)
    return [triple_span(n, (0, 1, 2)) + ("row",),
            (triple_span(n, run[0])[0], triple_span(n, run[-1])[1], "chunks"),
            triple_span(n, last) + ("last",)]


@pytest.fixture(scope="module", params=["wave", "host"])
def wide_engines(request):
    """(default GPU engine, CPU engine, ordered GPU engine), with the wave
    kernel forced for every pool, or with the kernel the host picks: at
    these pools the batch kernel's wide walk."""
    need_gpu()
    old = _core.scan5_wave_min_pool()
    if request.param == "wave":
        _core.set_scan5_wave_min_pool(_core.SCAN5_WIDE_MIN_ROW + 4)
    else:
        assert max(WIDE_POOLS) < old == _core.SCAN5_WAVE_MIN_POOL
    gpu, cpu = orc.make_pair(True)
    gpu_ord = orc.rijndael_engine(True, gpu="force", ordered=True)
    assert gpu.gpu_active and gpu_ord.gpu_active
    yield gpu, cpu, gpu_ord
    _core.set_scan5_wave_min_pool(old)


def check_wide(engines, n, name):
    """Returns (scans on the default engine, scans on the ordered one)."""
    gpu, cpu, gpu_ord = engines
    st = pool5(n)[0]
    target = aes_target()
    mask = orc.onesided_masks(target, one.MASK_SEED)[name]
    kw = dict(seed=orc.SCAN_SEED)
    ordered_scans = 3
    for begin, end, what in wide_windows(n):
        where = (n, name, what, begin, end)
        _, _, ev_c = cpu.scan_pool(5, st, target, mask, begin, end,
                                   count_all=True, **kw)
        _, _, ev_g = gpu.scan_pool(5, st, target, mask, begin, end,
                                   count_all=True, **kw)
        assert ev_g == ev_c == end - begin, where
        f_c, r_c, ev_c = cpu.scan_pool(5, st, target, mask, begin, end, **kw)
        f_g, r_g, ev_g = gpu.scan_pool(5, st, target, mask, begin, end, **kw)
        f_o, r_o, ev_o = gpu_ord.scan_pool(5, st, target, mask, begin, end,
                                           **kw)
        assert bool(f_g) == bool(f_c) == bool(f_o), where
        if not f_c:
            assert ev_g == ev_o == ev_c == end - begin, where
            continue
        assert list(r_o) == list(r_c), (where, list(r_o), list(r_c))
        for res in (r_g, r_o):
            orc.assert_hit_valid(5, st, res, target, mask)
            orc.assert_no_zero_function(5, res)
            assert begin <= orc.checked_rank(orc.hit_ids(5, res), n) < end
        # The ordered engine again from behind each of the next CPU hits.
        for _ in range(FOLLOW_UPS):
            begin = orc.checked_rank(orc.hit_ids(5, r_c), n) + 1
            if begin >= end:
                break
            f_c, r_c, _ = cpu.scan_pool(5, st, target, mask, begin, end, **kw)
            f_o, r_o, _ = gpu_ord.scan_pool(5, st, target, mask, begin, end,
                                            **kw)
            ordered_scans += 1
            assert bool(f_o) == bool(f_c), (where, begin)
            if not f_c:
                break
            assert list(r_o) == list(r_c), (where, begin, list(r_o), list(r_c))
    return 2 * 3, ordered_scans


@pytest.mark.parametrize("name", WIDE_MASKS)
@pytest.mark.parametrize("n", WIDE_POOLS)
def test_scan5_wide_and_wave(wide_engines, n, name):
    gpu, _, gpu_ord = wide_engines
    before = gpu.stats()["gpu_scans"], gpu_ord.stats()["gpu_scans"]
    scans = check_wide(wide_engines, n, name)
    check_ran_on_gpu(gpu, scans[0], before[0])
    check_ran_on_gpu(gpu_ord, scans[1], before[1])


# --- 4. whole nodes ---------------------------------------------------------

NODE_MASKS = ("Zall", "Oall", "E")


def run_node(sbox_name, lut, name, gpu):
    """create_circuit from the initial state, target bit 0 under the mask:
    (returned gate, state XML, stats)."""
    sbox, n = models.load(sbox_name)
    eng = make_engine(lut_graph=lut, seed=1, gpu=gpu, ordered=gpu == "force",
                      save_states=False)
    eng.set_sbox(sbox, n)
    st = eng.initial_state()
    target = eng.target(0)
    mask = orc.onesided_masks(target, one.MASK_SEED, n)[name]
    assert not orc.tt_int(mask) & ~orc.tt_int(mask_for_inputs(n))
    out = eng.create_circuit(st, target, mask)
    if out >= 0:
        # A returned gate realises the target under the mask.
        assert tt_eq_mask(target, st.gate(out)["table"], mask), (out, name)
    return out, st.to_xml(), eng.stats()


@pytest.mark.parametrize("name", NODE_MASKS)
@pytest.mark.parametrize("lut", [True, False], ids=["lut", "gates"])
@pytest.mark.parametrize("sbox_name", ["des_s1", "rijndael"])
def test_whole_node(monkeypatch, capfd, sbox_name, lut, name):
    need_gpu()
    monkeypatch.delenv("SBOXGATES_NO_SVC", raising=False)
    out_c, xml_c, stats_c = run_node(sbox_name, lut, name, "off")
    out_g, xml_g, stats = run_node(sbox_name, lut, name, "force")
    where = (sbox_name, lut, name)
    assert out_g == out_c, where
    assert xml_g == xml_c, where
    # Every scan of the CPU engine's search ran on the GPU here.
    assert stats["cpu_scans"] == 0, (where, stats)
    assert stats["gpu_scans"] == stats_c["cpu_scans"], (where, stats)
    assert stats["nodes"] == stats_c["nodes"], where
    # Gate mode scans its triples on the scan service.
    assert "scan service disabled" not in capfd.readouterr().err
    if not lut and name == "Zall":
        # No gate of the default set is constant 0 under the mask.
        assert out_c == -1, where
