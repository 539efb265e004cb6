"""The contract of include/memb_hip_query_bags.h restated in numpy, for the query-bags tests on both sides
(tests/test_query_bags_host.py, tests/test_gpu_query_bags.py): the composition of two references that exist already -- the
sequential pooling of tests/pooled_reference.py and the matrix of tests/query_matrix_reference.py over the pooled rows --,
a scalar restatement with pair_of_two_rows, the top-k through tests/query_topk_reference.py, and the batches those tests
share. Pure numpy: no torch, no GPU."""
import numpy as np

from bag_pairs_reference import bag_pair_lengths
from pairs_reference import pair_of_two_rows
from pooled_reference import clamped, ids_with_misses, offsets_of, pooled_by_the_contract
from query_matrix_reference import matrix_by_the_contract
from query_topk_reference import topk_by_the_contract


def query_bags_by_the_contract(queries, values, offsets, mode):
    """(cosines (Q, bags), dots (Q, bags), norms (bags,)), all float32. queries: float32 (Q, dim); values: the (n, dim)
    float32 rows of the entries (zeros for a missing one); offsets: bags + 1 entries, read as the kernels read them."""
    pooled = pooled_by_the_contract(np.ascontiguousarray(values, dtype=np.float32), offsets, mode)
    return matrix_by_the_contract(queries, pooled)


def query_bags_pair_by_pair(queries, values, offsets, mode):
    """query_bags_by_the_contract restated with scalars: a loop over queries and bags, each bag added entry by entry,
    pair_of_two_rows for each (query, bag)"""
    values = np.ascontiguousarray(values, dtype=np.float32)
    bounds = clamped(offsets, len(values))
    count, bags = len(queries), len(bounds) - 1
    cosines = np.zeros((count, bags), dtype=np.float32)
    dots = np.zeros((count, bags), dtype=np.float32)
    norms = np.zeros(bags, dtype=np.float32)
    for b in range(bags):
        begin, end = int(bounds[b]), int(bounds[b + 1])
        row = np.zeros(values.shape[1], dtype=np.float32)
        if end > begin:
            row = values[begin].copy()
            for i in range(begin + 1, end):
                row = np.add(row, values[i], dtype=np.float32)
            if mode == 'mean':
                row = np.divide(row, np.float32(end - begin), dtype=np.float32)
        for q in range(count):
            cosines[q, b], dots[q, b], _, norms[b] = pair_of_two_rows(queries[q], row)
        if not count:
            norms[b] = pair_of_two_rows(row, row)[3]
    return cosines, dots, norms


def query_bags_topk_by_the_contract(queries, values, offsets, mode, k):
    """(values (Q, k), positions (Q, k)): the order of tests/query_topk_reference.py over the matrix above"""
    return topk_by_the_contract(query_bags_by_the_contract(queries, values, offsets, mode)[0], k)


def bags_batch(words, bags, n_rows, seed):
    """(rows, offsets): `bags` bags with the lengths of bag_pair_lengths for `words` words per wavefront -- 0, 1, W - 1, W,
    W + 1, 2 W + 1, one bag of 300 from 17 bags on --, ids from ids_with_misses; bag 0 holds known rows only"""
    offsets = offsets_of(bag_pair_lengths(words, (bags + 1) // 2, seed)[:bags])
    rows = ids_with_misses(int(offsets[-1]), n_rows, seed)
    if bags:
        rows[:int(offsets[1])] %= np.uint32(n_rows)
    return rows, offsets


def queries_batch(count, dim, seed, values=None):
    """float32 (count, dim) queries; where `values` (entry rows) are given, query 1 is the first of them and query 2 its
    negation"""
    queries = np.random.default_rng(seed).standard_normal((count, dim)).astype(np.float32)
    if values is not None and len(values):
        if count > 1:
            queries[1] = values[0]
        if count > 2:
            queries[2] = -values[0]
    return queries
