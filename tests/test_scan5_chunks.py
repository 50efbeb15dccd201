"""Chunk rule of k_scan5_wave's triple queue (sbg/scan5_geom.hpp), on the
CPU: the chunks that the waves take with one atomic each partition the
queue's triples exactly, come in increasing order and never hold more
triples than a wave has lanes to decode them."""

import math

import pytest

from sboxgates_amd import _core

CHUNK_MAX = _core.SCAN5_CHUNK_MAX
CHUNK_MIN = _core.SCAN5_CHUNK_MIN
# Waves of the grids the host launches: 4 per block, up to 2048 blocks.
WAVES = (4, 12, 64, 1000, 4 * 2048)


def test_chunk_max_is_a_wave():
    assert CHUNK_MAX == 64


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("n", [44, 65, 130, 450, 500])
def test_chunks_partition_the_triples(n, waves):
    units = math.comb(n, 3)
    chunks = _core.scan5_chunks(units, waves)
    at = 0
    for first, count in chunks:
        assert first == at, (n, waves, first, at)  # increasing, no gap
        assert 1 <= count <= CHUNK_MAX, (n, waves, first, count)
        at += count
    assert at == units, (n, waves, at, units)


@pytest.mark.parametrize("waves", WAVES)
@pytest.mark.parametrize("units", [0, 1, 2, 63, 64, 65, 1000, 8 * 64 * 12 + 5])
def test_short_queues(units, waves):
    """Queues of a window inside the pool: any length, also none."""
    chunks = _core.scan5_chunks(units, waves)
    assert sum(c for _, c in chunks) == units
    assert [f for f, _ in chunks] == [
        sum(c for _, c in chunks[:i]) for i in range(len(chunks))]
    assert all(1 <= c <= CHUNK_MAX for _, c in chunks)


@pytest.mark.parametrize("n", [65, 130, 450])
def test_small_scans_keep_small_chunks(n):
    """On the grid the host launches (a wave per CHUNK_MIN triples, at most
    2048 blocks) every wave gets a chunk, so all blocks get work, and no
    chunk but the bulk's last is smaller than CHUNK_MIN: a queue serves its
    atomics one at a time. A large scan takes whole waves of triples and
    ends in chunks of CHUNK_MIN."""
    units = math.comb(n, 3)
    waves = 4 * min(2048, units // (4 * CHUNK_MIN) + 1)
    chunks = _core.scan5_chunks(units, waves)
    assert len(chunks) >= waves - 4
    sizes = [c for _, c in chunks]
    assert sum(1 for s in sizes if s < CHUNK_MIN) <= 1
    if n != 450:
        assert max(sizes) == CHUNK_MIN
    if n == 450:
        assert sizes[0] == CHUNK_MAX
        assert sizes[-1] == CHUNK_MIN
        # The sizes only fall, but for one short chunk that ends the bulk.
        steps = [b for a, b in zip(sizes, sizes[1:]) if b != a]
        assert all(s < CHUNK_MAX for s in steps)
        tail = sizes[sizes.index(CHUNK_MAX // 2, 1):]
        assert tail == sorted(tail, reverse=True)
