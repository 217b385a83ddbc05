"""GPU tests of the many-keys work-list sort (sort_kernels.h k_sort_tilehist / k_sort_tilescatter / k_sort_plan / k_sort_segments), through
artis_amd_debug_sort_list on the engine of a 5^3 model. Every case asserts that the output is a permutation of the list and that the keys of
its entries, read back through each entry's position in the input, are non-decreasing. The order among equal keys is free.

Shapes: the lengths at which the host's launch arithmetic or a kernel's loop bounds change (the shortest sorted list 2*BLOCK, one tile of pass 1
= one chunk of pass 2 = 8192 entries, each +-1, a few tiles and a ragged end at 100 003); the key counts of the headline's thermal and r-packet
lists, the first count above the few-keys path, 2^22, and the largest the sort takes (2^25, whose pass 2 needs 128 KB of LDS); key patterns
that put everything into one bucket, one digit, the two ends, the two sides of every bucket boundary, and the skewed list whose one bucket is
cut into 123 chunks."""
import time

import numpy as np
import pytest

from artis_amd import synth

pytestmark = pytest.mark.gpu

BLOCK = 256           # artis_engine.hip BLOCK: a list below 2 * BLOCK stays as it is
TILE = 8192           # SORT_TILE = SORT_SEG_CAP
SORT_LDS_KEYS = 8192  # up to here the few-keys path sorts
HI_BITS = 11          # SORT_HI_BITS: pass 1 has at most 2^11 buckets
MAX_KEYS = 1 << 25    # SORT_MAX_KEYS
ERR_ARG, ERR_UNSUPPORTED = -3, -4
NKEYS = [SORT_LDS_KEYS + 1, 125000 * 16, 125000 * 32, 1 << 22, MAX_KEYS]
LENGTHS = [2 * BLOCK, 2 * BLOCK + 1, TILE - 1, TILE, TILE + 1, 100_003]


def bucket_width(nkeys: int) -> int:
    """keys per pass-1 bucket (sort_many_keys: the low digit takes the bits that 2^HI_BITS buckets leave over)"""
    return 1 << max(0, int(nkeys - 1).bit_length() - HI_BITS)


@pytest.fixture(scope="module")
def eng():
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from artis_amd import engine

    e = engine.Engine(synth.build("small", ncoord=5)[0])
    yield e
    e.close()


def check_sorted(eng, keys, nkeys, what):
    """sort a list of distinct entries (so that an entry names its position in the input) and assert the two properties"""
    keys = np.asarray(keys, dtype=np.int32)
    n = len(keys)
    rng = np.random.default_rng(n + nkeys)
    lst = (rng.permutation(n) if n else np.zeros(0)).astype(np.int32) * 3 + 7  # entries are not their own positions
    out = eng.debug_sort_list(keys, lst, nkeys)
    assert out.shape == lst.shape
    assert np.array_equal(np.sort(out), np.sort(lst)), f"{what}: the output is not a permutation of the list"
    pos = np.empty(n * 3 + 8, dtype=np.int64)
    pos[lst] = np.arange(n)
    k = keys[pos[out]]
    bad = np.flatnonzero(k[1:] < k[:-1])
    assert bad.size == 0, f"{what}: keys decrease at {bad[:5]} of {n} (keys {k[bad[:5]]} -> {k[bad[:5] + 1]})"
    return out, lst


@pytest.mark.parametrize("nkeys", NKEYS)
@pytest.mark.parametrize("n", LENGTHS)
def test_uniform_random_keys(eng, n, nkeys):
    keys = np.random.default_rng(1000 + n).integers(0, nkeys, n)
    check_sorted(eng, keys, nkeys, f"uniform n={n} nkeys={nkeys}")


@pytest.mark.parametrize("n", [0, 1, 2 * BLOCK - 1])
def test_short_list_stays_as_it_is(eng, n):
    keys = np.random.default_rng(n).integers(0, 1 << 22, n)
    out, lst = check_sorted_or_unsorted(eng, keys, 1 << 22)
    assert np.array_equal(out, lst)


def check_sorted_or_unsorted(eng, keys, nkeys):
    keys = np.asarray(keys, dtype=np.int32)
    lst = np.arange(len(keys), dtype=np.int32)[::-1].copy()
    return eng.debug_sort_list(keys, lst, nkeys), lst


@pytest.mark.parametrize("nkeys", NKEYS)
def test_key_patterns(eng, nkeys):
    n = 100_003
    B = bucket_width(nkeys)
    rng = np.random.default_rng(nkeys)
    for name, keys in [
        ("all key 0", np.zeros(n)),
        ("all one middle key", np.full(n, nkeys // 2)),
        ("all the last key", np.full(n, nkeys - 1)),
        ("the two extreme keys", np.where(rng.integers(0, 2, n) == 1, nkeys - 1, 0)),
        ("already sorted", np.sort(rng.integers(0, nkeys, n))),
        ("reverse sorted", np.sort(rng.integers(0, nkeys, n))[::-1]),
    ]:
        check_sorted(eng, keys, nkeys, f"{name}, nkeys={nkeys}")
    # both sides of every bucket boundary: k*B - 1 and k*B for every k (and nothing else), in random order
    edges = np.arange(1, (nkeys - 1) // B + 1) * B
    edges = np.concatenate([edges - 1, edges])
    edges = edges[edges < nkeys]
    keys = rng.permutation(np.resize(edges, max(n, 2 * len(edges))))
    check_sorted(eng, keys, nkeys, f"bucket boundaries, nkeys={nkeys}")


@pytest.mark.parametrize("nkeys", [125000 * 32, MAX_KEYS])
def test_skewed_list(eng, nkeys):
    """one bucket holds all but 100 of 1 000 003 entries: pass 2 cuts it into chunks, and the sort stays a matter of milliseconds"""
    n = 1_000_003
    B = bucket_width(nkeys)
    rng = np.random.default_rng(7)
    b = (nkeys // B) // 2
    keys = rng.integers(b * B, (b + 1) * B, n)
    keys[rng.choice(n, 100, replace=False)] = rng.integers(0, nkeys, 100)
    t0 = time.perf_counter()
    check_sorted(eng, keys, nkeys, f"skewed, nkeys={nkeys}")
    assert time.perf_counter() - t0 < 5.0  # (the copies and the host's checks included: the sort itself takes well under a millisecond)


def test_two_sorts_in_a_row(eng):
    """nothing of one sort's scratch (the engine's, which the entry point uses) shows in the next: a long list with many keys, a short one with
    few, a third shape"""
    rng = np.random.default_rng(11)
    a = rng.integers(0, 1 << 22, 100_003)
    b = rng.integers(0, SORT_LDS_KEYS + 1, 2 * BLOCK + 1)
    check_sorted(eng, a, 1 << 22, "first")
    check_sorted(eng, b, SORT_LDS_KEYS + 1, "second")
    check_sorted(eng, a[:TILE + 1] % (125000 * 16), 125000 * 16, "third")


def test_unsupported_key_counts_are_refused(eng):
    from artis_amd.engine import EngineError

    keys = np.zeros(1000, dtype=np.int32)
    with pytest.raises(EngineError, match=f"error {ERR_UNSUPPORTED}.*at most {MAX_KEYS} keys"):
        eng.debug_sort_list(keys, keys, MAX_KEYS + 1)
    with pytest.raises(EngineError, match=f"error {ERR_ARG}.*above {SORT_LDS_KEYS}"):
        eng.debug_sort_list(keys, keys, SORT_LDS_KEYS)
    with pytest.raises(EngineError, match=f"error {ERR_ARG}.*outside"):
        eng.debug_sort_list(keys + (1 << 22), keys, 1 << 22)
