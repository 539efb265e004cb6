"""The contracts of include/memb_hip_analogies.h in numpy. The selection with an exclusion list is the contract of the
selection itself (query_topk_reference.topk_by_the_contract) over each row WITHOUT its excluded columns, the positions mapped
back; the weighted sum is a loop of float32 multiplies and adds in entry order."""
import numpy as np

from query_topk_reference import EMPTY_POSITION, EMPTY_VALUE, topk_by_the_contract


def topk_excluding_by_the_contract(matrix, k, excluded, base=0):
    """(values float32 (Q, k) with the matrix's bits, positions int64 (Q, k)); excluded: integer (Q, E) positions
    (base + column), any order, repeats allowed, entries outside [base, base + n) ignored; None: no list"""
    matrix = np.ascontiguousarray(matrix, dtype=np.float32)
    count, n = matrix.shape
    values = np.full((count, k), EMPTY_VALUE, dtype=np.float32)
    positions = np.full((count, k), EMPTY_POSITION, dtype=np.int64)
    for q in range(count):
        named = set() if excluded is None else {int(entry) - base for entry in np.asarray(excluded)[q]}
        kept = np.array([column for column in range(n) if column not in named], dtype=np.int64)
        got = topk_by_the_contract(matrix[q:q + 1, kept], k)
        found = got[1][0] >= 0
        values.view(np.uint32)[q] = got[0].view(np.uint32)[0]
        positions[q, found] = base + kept[got[1][0, found]]
    return values, positions


def drop_by_stable_sort(values, positions, excluded, k):
    """what most_similar_device does with its own row, for a whole list: the entries whose position the row's list names go
    behind the others by a stable sort, the first k stay"""
    named = (positions[:, :, None] == np.asarray(excluded, dtype=np.int64)[:, None, :]).any(axis=2) & (positions >= 0)
    order = np.argsort(named, axis=1, kind='stable')[:, :k]
    return np.take_along_axis(values, order, axis=1), np.take_along_axis(positions, order, axis=1)


def weighted_rows_sum_reference(matrix, weights, offsets):
    """float32 (Q, dim): out[q] = out[q] + (weights[e] * matrix[e]) over e = offsets[q] .. offsets[q + 1], from +0.0, the
    product and the sum each rounded to float32; weights None: all +1"""
    matrix = np.ascontiguousarray(matrix, dtype=np.float32)
    offsets = [int(offset) for offset in offsets]
    out = np.zeros((len(offsets) - 1, matrix.shape[1]), dtype=np.float32)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        for q in range(len(offsets) - 1):
            total = np.zeros(matrix.shape[1], dtype=np.float32)
            for entry in range(offsets[q], offsets[q + 1]):
                weight = np.float32(1.0) if weights is None else np.float32(weights[entry])
                product = (weight * matrix[entry]).astype(np.float32)
                total = (total + product).astype(np.float32)
            out[q] = total
    return out
