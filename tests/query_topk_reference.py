"""The contract of include/memb_hip_query_topk.h in numpy, twice: vectorised (topk_by_the_contract) and as a scalar
restatement that compares two entries the way the header words it (topk_entry_by_entry). Row q of the matrix ordered by a
stable descending sort -- a greater value first, NaN greater than every number, equal values (-0.0 == +0.0, NaN == NaN) lower
position first --, cut to k; positions as base + column; -inf and -1 in the slots from min(k, n) on."""
import functools

import numpy as np

EMPTY_VALUE = np.float32(-np.inf)
EMPTY_POSITION = -1


def topk_by_the_contract(matrix, k, base=0):
    """(values float32 (Q, k) with the matrix's bits, positions int64 (Q, k))"""
    matrix = np.ascontiguousarray(matrix, dtype=np.float32)
    count, n = matrix.shape
    nan = np.isnan(matrix)
    # ranks that are equal exactly where the contract's values are equal: NaN above +inf, the zeros together
    rank = np.where(nan, np.inf, matrix.astype(np.float64) + 0.0)
    tie = np.where(nan, 1, 0)
    # stable, ascending in (-tie, -rank): the greater first, equal ones in the order of their positions
    order = np.lexsort((np.broadcast_to(np.arange(n), (count, n)), -rank, -tie), axis=1)[:, :k]
    values = np.full((count, k), EMPTY_VALUE, dtype=np.float32)
    positions = np.full((count, k), EMPTY_POSITION, dtype=np.int64)
    found = order.shape[1]
    values.view(np.uint32)[:, :found] = np.take_along_axis(matrix.view(np.uint32), order, axis=1)
    positions[:, :found] = base + order
    return values, positions


def comes_before(a, b):
    """entry a = (value, position) comes before entry b, in the header's words"""
    (x, i), (y, j) = a, b
    x_nan, y_nan = bool(np.isnan(x)), bool(np.isnan(y))
    if x_nan != y_nan:
        return x_nan                       # NaN counts as greater than every number
    if not x_nan and float(x) != float(y):
        return float(x) > float(y)         # a greater value comes first (-0.0 == +0.0)
    return i < j                           # equal values: the lower position first


def topk_entry_by_entry(matrix, k, base=0):
    matrix = np.ascontiguousarray(matrix, dtype=np.float32)
    count, n = matrix.shape
    values = np.full((count, k), EMPTY_VALUE, dtype=np.float32)
    positions = np.full((count, k), EMPTY_POSITION, dtype=np.int64)
    compare = functools.cmp_to_key(lambda a, b: -1 if comes_before(a, b) else (1 if comes_before(b, a) else 0))
    for q in range(count):
        entries = sorted(((matrix[q, i], i) for i in range(n)), key=compare)[:k]
        for j, (value, i) in enumerate(entries):
            values[q, j] = value
            values.view(np.uint32)[q, j] = matrix.view(np.uint32)[q, i]
            positions[q, j] = base + i
    return values, positions


def same_topk(got, want):
    """values as bits, positions equal"""
    return (got[0].shape == want[0].shape and got[1].shape == want[1].shape and got[1].dtype == np.int64
            and np.array_equal(np.ascontiguousarray(got[0]).view(np.uint32), np.ascontiguousarray(want[0]).view(np.uint32))
            and np.array_equal(got[1], want[1]))


def rows_of_every_kind(n, seed=0):
    """(name, float32 (n,) row): ascending (every element inserts), descending, constant (all ties), +0.0 / -0.0 mixed, NaNs
    among numbers, real -inf entries, and Gaussian values with repeats"""
    rng = np.random.default_rng(seed + n)
    ramp = np.arange(n, dtype=np.float32) / np.float32(max(n, 1))
    zeros = np.where(rng.integers(0, 2, size=n) == 1, np.float32(-0.0), np.float32(0.0)).astype(np.float32)
    with_nan = rng.standard_normal(n).astype(np.float32)
    with_nan[rng.integers(0, 3, size=n) == 0] = np.nan
    if n > 1:
        with_nan.view(np.uint32)[n // 2] = 0xFFC12345   # a negative NaN with a payload of its own
    minus_inf = rng.standard_normal(n).astype(np.float32)
    minus_inf[rng.integers(0, 2, size=n) == 0] = -np.inf
    repeats = np.round(rng.standard_normal(n) * 3).astype(np.float32) / np.float32(3)
    return [('ascending', ramp), ('descending', -ramp), ('constant', np.full(n, 0.25, dtype=np.float32)), ('zeros', zeros),
            ('nan', with_nan), ('minus inf', minus_inf), ('all minus inf', np.full(n, -np.inf, dtype=np.float32)),
            ('repeats', repeats)]
