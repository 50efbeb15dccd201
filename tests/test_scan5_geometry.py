"""Task geometry of k_scan5's wide walk (sbg/scan5_geom.hpp), checked on the
CPU through _core.scan5_wide_tasks: the kernel calls the same functions.

A task is (row d, real id of the gate on bit 0 of its 64-gate word group,
valid mask). Word groups are aligned to the pool's end, so the gate on bit 0
of the lowest group has a negative id when the pool is no multiple of the
group size. For every triple (named by its last gate c) the valid bits of
its tasks must be exactly the pairs (d, e), c < d < e < n, that lie in the
window of flat pair indices and hold no excluded gate, each once.
"""

import functools
import random

import pytest

from sboxgates_amd import _core

GB = _core.SCAN5_WIDE_GB
SMALL = (44, 64, 65, 70, 127, 128, 129)
LARGE = (450, 500)


def cs_of(n):
    """Every c at the small pools, a spread at the large ones."""
    if n in SMALL:
        return list(range(n - 2))
    pad = _core.scan5_wide_pad(n)
    edges = set()
    # The triple's first group changes at c + pad + 2 = GB k.
    for k in range(0, n + pad, GB):
        edges.update(k - pad + j for j in (-3, -2, -1))
    edges.update((0, n - 4, n - 3))
    edges.update(random.Random(n).sample(range(n - 2), 4))
    return sorted(c for c in edges if 0 <= c <= n - 3)


@functools.lru_cache(maxsize=4)
def pairs(n, c):
    """The pairs behind c in d-major order: a pair's flat index is its
    position in this list."""
    return [(d, e) for d in range(c + 1, n - 1) for e in range(d + 1, n)]


def covered(n, c, lo, hi, excl=0):
    """Pairs named by the valid bits of the triple's tasks, as a list."""
    pad = _core.scan5_wide_pad(n)
    out = []
    for d, e0, valid in _core.scan5_wide_tasks(n, c, lo, hi, excl):
        assert 0 <= valid < 1 << GB
        assert (e0 + pad) % GB == 0
        while valid:
            low = valid & -valid
            out.append((d, e0 + low.bit_length() - 1))
            valid ^= low
    return out


def expected(n, c, lo, hi, excl=0):
    window = pairs(n, c)[lo:hi]
    if excl == 0:
        return window
    gone = {g for g in range(64) if (excl >> g) & 1}
    return [p for p in window if p[0] not in gone and p[1] not in gone]


def closed_form_count(n, c):
    """Rows that have an e > d in the group, summed over end-aligned groups
    (counted directly, not with the header's formula)."""
    pad = _core.scan5_wide_pad(n)
    total = 0
    for g in range((n + pad) // GB):
        top = min(GB * g + GB - 1 - pad, n - 1)  # the group's last real gate
        total += max(0, min(n - 2, top - 1) - c)
    return total


@pytest.mark.parametrize("n", SMALL + LARGE)
def test_pad(n):
    pad = _core.scan5_wide_pad(n)
    assert 0 <= pad < GB and (n + pad) % GB == 0


@pytest.mark.parametrize("n", SMALL + LARGE)
def test_full_window_covers_every_pair_once(n):
    for c in cs_of(n):
        m = n - 1 - c
        npairs = m * (m - 1) // 2
        tasks = _core.scan5_wide_tasks(n, c, 0, npairs, 0)
        assert len(tasks) == closed_form_count(n, c), (n, c)
        # No task is empty under the full window: none is wasted.
        assert all(valid != 0 for _, _, valid in tasks), (n, c)
        got = covered(n, c, 0, npairs)
        assert len(got) == len(set(got)) == npairs, (n, c)
        assert sorted(got) == expected(n, c, 0, npairs), (n, c)


@pytest.mark.parametrize("n", SMALL + LARGE)
def test_random_windows(n):
    rng = random.Random(0x5CA + n)
    for c in cs_of(n):
        m = n - 1 - c
        npairs = m * (m - 1) // 2
        for _ in range(3 if n in SMALL else 2):
            lo = rng.randrange(npairs + 1)
            hi = rng.randrange(lo, npairs + 1)
            got = covered(n, c, lo, hi)
            assert len(got) == len(set(got)), (n, c, lo, hi)
            assert sorted(got) == expected(n, c, lo, hi), (n, c, lo, hi)
        assert covered(n, c, npairs, npairs) == []


@pytest.mark.parametrize("n", SMALL + LARGE)
def test_random_exclusions(n):
    rng = random.Random(0xE8C + n)
    pad = _core.scan5_wide_pad(n)
    # The real ids on shifted bits 63 and 64, where the mask's shift turns.
    edge = {g for g in (0, 63 - pad, 64 - pad, 63) if 0 <= g < 64}
    for c in cs_of(n):
        m = n - 1 - c
        npairs = m * (m - 1) // 2
        sets = [sum(1 << g for g in edge), 1 << 63, ~0 & (2**64 - 1),
                rng.getrandbits(64), rng.getrandbits(64) & rng.getrandbits(64)]
        for excl in sets[:5 if n in SMALL else 3]:
            got = covered(n, c, 0, npairs, excl)
            assert len(got) == len(set(got)), (n, c, hex(excl))
            assert sorted(got) == expected(n, c, 0, npairs, excl), (n, c,
                                                                   hex(excl))
        # Exclusion and a window together.
        excl = rng.getrandbits(64)
        lo = rng.randrange(npairs + 1)
        hi = rng.randrange(lo, npairs + 1)
        assert sorted(covered(n, c, lo, hi, excl)) == expected(
            n, c, lo, hi, excl), (n, c, lo, hi, hex(excl))


def test_bad_arguments():
    with pytest.raises(ValueError):
        _core.scan5_wide_tasks(70, 68, 0, 1, 0)
    with pytest.raises(ValueError):
        _core.scan5_wide_tasks(2, 0, 0, 1, 0)
