"""The contract of include/memb_hip_queries.h restated in numpy, for the query tests on both sides
(tests/test_queries_host.py, tests/test_gpu_queries.py): pairs_by_the_contract of tests/pairs_reference.py over the pair
(query of the entry's group, the entry's fp32 row) -- nothing else --, the map from entries to groups as the kernel reads
the offsets (clamped to n), and the batches those tests share. Pure numpy: no torch, no GPU."""
import numpy as np

from pairs_reference import pair_of_two_rows, pairs_by_the_contract
from pooled_reference import ids_with_misses, offsets_of

LONG_GROUP = 300   # entries of the one long group of a batch of many groups


def groups_of_entries(offsets, n):
    """(group (n,) int64, inside (n,) bool) for ascending offsets of G + 1 entries, read as uint32 and clamped to n: entry i
    lies in the last group g with offsets[g] <= i, and in none (inside False) before offsets[0] and from offsets[G] on"""
    clamped = np.minimum(np.asarray(offsets).astype(np.int64) & 0xFFFFFFFF, n)
    assert (clamped[1:] >= clamped[:-1]).all(), 'defined for non-decreasing offsets'
    group = np.searchsorted(clamped, np.arange(n, dtype=np.int64), side='right') - 1
    inside = (group >= 0) & (group < len(clamped) - 1)
    return group, inside


def queries_by_the_contract(queries, values, offsets):
    """(cosines (n,), dots (n,), norms (n,), inside (n,)): the pair contract over (queries[group of i], values[i]) for every
    entry that lies in a group, float32; +0.0 where inside is False (such an entry is not written). queries: float32
    (G, dim); values: the (n, dim) float32 rows of the entries (zeros for a missing one)."""
    queries = np.ascontiguousarray(queries, dtype=np.float32)
    values = np.ascontiguousarray(values, dtype=np.float32)
    n = values.shape[0]
    group, inside = groups_of_entries(offsets, n)
    cosines, dots, norms = (np.zeros(n, dtype=np.float32) for _ in range(3))
    chosen = np.flatnonzero(inside)
    if chosen.size:
        cosines[chosen], dots[chosen], both = pairs_by_the_contract(queries[group[chosen]], values[chosen])
        norms[chosen] = both[:, 1]
    return cosines, dots, norms, inside


def queries_entry_by_entry(queries, values, offsets):
    """queries_by_the_contract restated with scalars: a loop over groups and entries, pair_of_two_rows for each"""
    n = len(values)
    clamped = [min(int(value) & 0xFFFFFFFF, n) for value in offsets]
    cosines, dots, norms = (np.zeros(n, dtype=np.float32) for _ in range(3))
    inside = np.zeros(n, dtype=bool)
    for g in range(len(clamped) - 1):
        for i in range(clamped[g], clamped[g + 1]):
            cosines[i], dots[i], _, norms[i] = pair_of_two_rows(queries[g], values[i])
            inside[i] = True
    return cosines, dots, norms, inside


def group_lengths(words, groups, seed):
    """The lengths of the groups of a batch for a geometry of `words` words per wavefront (W): 0, 1, W - 1, W, W + 1 and
    3 W + 1 mixed so that group ends fall inside tiles. The first groups are fixed -- a batch of one, two or three groups
    still holds edges --: an EMPTY FIRST group, a tile and one word, three empty groups IN A ROW, one word, W - 1, 3 W + 1, W,
    the long group; the LAST group of a batch of more than three is empty."""
    small = max(words - 1, 1)
    core = [0, words + 1, 3 * words + 1, 0, 0, 0, 1, small, words, LONG_GROUP, words + 1, 1]
    rng = np.random.default_rng(seed)
    choices = np.array([0, 1, small, words, words + 1, 3 * words + 1])
    drawn = choices[rng.integers(0, len(choices), size=max(groups - len(core), 0))]
    lengths = np.concatenate([np.array(core, dtype=np.int64), drawn])[:groups]
    if groups > 3:
        lengths[-1] = 0
    return lengths


def query_batch(words, groups, dim, n_rows, seed, head=0, tail=0):
    """(queries (groups, dim) float32, rows, offsets): Gaussian queries, groups of group_lengths, ids from ids_with_misses
    (0xFFFFFFFF and ids >= n_rows among them). head / tail: entries in front of offsets[0] / from offsets[groups] on, which lie
    in no group."""
    offsets = offsets_of(group_lengths(words, groups, seed)) + head
    n = int(offsets[-1]) + tail
    rows = ids_with_misses(n, n_rows, seed) if n else np.zeros(0, dtype=np.uint32)
    if n:
        rows[:min(n, 8)] %= np.uint32(n_rows)   # (known rows in front: no batch is all zeros)
    queries = np.random.default_rng(seed + 77).standard_normal((groups, dim)).astype(np.float32)
    return queries, rows, offsets
