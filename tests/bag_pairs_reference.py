"""The contract of include/memb_hip_bag_pairs.h restated in numpy, for the bag-pair tests on both sides
(tests/test_bag_pairs_host.py, tests/test_gpu_bag_pairs.py): the composition of two references that exist already -- the
sequential pooling of tests/pooled_reference.py (a bag's rows added in entry order, one division for the mean, +0.0 for an
empty bag) and the pair reduction of tests/pairs_reference.py over the pooled rows of the bags 2j and 2j + 1 -- and the
batches those tests share. Pure numpy: no torch, no GPU."""
import numpy as np

from pairs_reference import pairs_by_the_contract
from pooled_reference import ids_with_misses, offsets_of, pooled_by_the_contract

LONG_BAG = 300      # entries of the one long bag of a batch
SELF_PAIR = 5       # the pair of bag_pairs_batch whose two bags hold the same ids


def bag_pairs_by_the_contract(values, offsets, mode):
    """(cosines (pairs,), dots (pairs,), norms (pairs, 2)), all float32. values: the (n, dim) float32 rows of the entries
    (zeros for a missing one); offsets: 2 * pairs + 1 entries, read as the kernels read them."""
    assert len(offsets) % 2 == 1
    pooled = pooled_by_the_contract(np.ascontiguousarray(values, dtype=np.float32), offsets, mode)
    return pairs_by_the_contract(pooled[0::2], pooled[1::2])


def bag_pair_lengths(words, pairs, seed):
    """The lengths of the 2 * pairs bags of a batch for a geometry of `words` words per wavefront (W): drawn from 0, 1,
    W - 1, W, W + 1 and 2 W + 1, with one bag of LONG_BAG entries. The first pairs are fixed, so that a batch of one, two or
    three pairs still holds the edges: a first bag that ends exactly on a tile boundary (pair 0: the batch starts on one),
    pairs that straddle one (pairs 0, 1, 6, 7), an empty-nonempty pair (1), an empty-empty pair (3), a bag against itself
    (SELF_PAIR), the long bag (8), and behind a filler pair that ends on a multiple of W another first bag of exactly one
    tile (10)."""
    small = max(words - 1, 1)
    core = [(words, words + 1), (0, 2 * words + 1), (small, 1), (0, 0), (0, 3), (5, 5), (2 * words + 1, words),
            (words + 1, words + 1), (LONG_BAG, 7)]
    so_far = sum(a + b for a, b in core)
    core += [(1, (-so_far - 1) % words), (words, small), (1, 0)]
    assert (sum(a + b for a, b in core[:10])) % words == 0 and core[SELF_PAIR][0] == core[SELF_PAIR][1]
    rng = np.random.default_rng(seed)
    choices = np.array([0, 1, small, words, words + 1, 2 * words + 1])
    drawn = choices[rng.integers(0, len(choices), size=(max(pairs - len(core), 0), 2))]
    lengths = np.concatenate([np.array(core, dtype=np.int64).reshape(-1, 2), drawn.reshape(-1, 2)])[:pairs]
    return lengths.reshape(-1)


def bag_pairs_batch(words, pairs, n_rows, seed):
    """(rows, offsets): `pairs` pairs of bags with the lengths of bag_pair_lengths, ids from ids_with_misses (0xFFFFFFFF and
    ids >= n_rows among them); the two bags of pair SELF_PAIR hold the same ids."""
    offsets = offsets_of(bag_pair_lengths(words, pairs, seed))
    rows = ids_with_misses(int(offsets[-1]), n_rows, seed)
    if pairs:
        rows[:int(offsets[2])] %= np.uint32(n_rows)   # (pair 0 of known rows only: no batch is all zeros)
    if pairs > SELF_PAIR:
        first, second, end = (int(offsets[2 * SELF_PAIR + k]) for k in range(3))
        rows[first:second] = np.arange(1, 1 + second - first)   # (known rows: the pair's cosine is 1)
        rows[second:end] = rows[first:second]
    return rows, offsets


def entry_values(reader, rows):
    """the float32 (n, dim) rows of the entries from the reader's own host decode, (0, dim) for none"""
    rows = np.asarray(rows, dtype=np.uint32)
    return reader.rows_embedding(rows) if len(rows) else np.zeros((0, reader.dim), dtype=np.float32)
