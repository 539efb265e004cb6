"""The contract of include/memb_hip_query_matrix.h restated in numpy, for the query-matrix tests on both sides
(tests/test_query_matrix_host.py, tests/test_gpu_query_matrix.py): pairs_by_the_contract of tests/pairs_reference.py over
every (query, row) -- nothing else --, and a scalar restatement with pair_of_two_rows. Pure numpy: no torch, no GPU."""
import numpy as np

from pairs_reference import pair_of_two_rows, pairs_by_the_contract


def matrix_by_the_contract(queries, values):
    """(cosines (Q, n), dots (Q, n), norms (n,)): the pair contract over (queries[q], values[i]) for every q and i, float32.
    queries: float32 (Q, dim); values: the (n, dim) float32 rows of the candidates (zeros for a missing one)."""
    queries = np.ascontiguousarray(queries, dtype=np.float32)
    values = np.ascontiguousarray(values, dtype=np.float32)
    count, n = queries.shape[0], values.shape[0]
    cosines = np.zeros((count, n), dtype=np.float32)
    dots = np.zeros((count, n), dtype=np.float32)
    norms = np.zeros(n, dtype=np.float32)
    for q in range(count):
        if n:
            cosines[q], dots[q], both = pairs_by_the_contract(np.repeat(queries[q:q + 1], n, axis=0), values)
            norms = both[:, 1].copy()
    if n and not count:
        norms = pairs_by_the_contract(values, values)[2][:, 1].copy()
    return cosines, dots, norms


def matrix_pair_by_pair(queries, values):
    """matrix_by_the_contract restated with scalars: a loop over queries and rows, pair_of_two_rows for each"""
    count, n = len(queries), len(values)
    cosines = np.zeros((count, n), dtype=np.float32)
    dots = np.zeros((count, n), dtype=np.float32)
    norms = np.zeros(n, dtype=np.float32)
    for q in range(count):
        for i in range(n):
            cosines[q, i], dots[q, i], _, norms[i] = pair_of_two_rows(queries[q], values[i])
    return cosines, dots, norms
