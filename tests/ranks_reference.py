"""include/memb_hip_ranks.h restated by brute force, sharing no code with memb_amd.reader.ranks_host: per row the named
columns are dropped, the rest is SORTED into the selection's order (key descending, position ascending) together with the
mark, and the answer is how many entries sort before the mark."""
import numpy as np

INT64_MAX = np.iinfo(np.int64).max


def key_of(value):
    """the selection's order on one float32 value as an integer, spelled out case by case"""
    value = np.float32(value)
    if np.isnan(value):
        return 0xFFFFFFFF
    if value == 0:
        return 0x80000000   # (-0.0 and +0.0)
    bits = int(value.view(np.uint32))
    return (~bits) & 0xFFFFFFFF if bits & 0x80000000 else bits | 0x80000000


def ranks_by_the_contract(matrix, thresholds, marks, base=0, exclude=None):
    """int64 (Q,): the counts of the float32 (Q, n) matrix, a column c being the position base + c"""
    matrix = np.asarray(matrix, dtype=np.float32)
    count, n = matrix.shape
    counts = np.zeros(count, dtype=np.int64)
    for q in range(count):
        dropped = set() if exclude is None else {int(entry) - base for entry in exclude[q]}
        columns = [c for c in range(n) if c not in dropped]
        # The mark goes in as one more entry. Its position is cut to base - 1 .. base + n, which changes its place among
        # the positions base .. base + n - 1 of the columns in no way and keeps the sums below inside int64. An entry with
        # the mark's key AND position does not precede it, so among such equals the mark is put first.
        mark = min(max(int(marks[q]), base - 1), base + n)
        keys = np.array([key_of(matrix[q, c]) for c in columns] + [key_of(thresholds[q])], dtype=np.int64)
        positions = np.array([base + c for c in columns] + [mark], dtype=np.int64)
        is_mark = np.array([1] * len(columns) + [0], dtype=np.int64)
        order = np.lexsort((is_mark, positions, -keys))
        counts[q] = int(np.nonzero(order == len(columns))[0][0])
    return counts


def hostile_matrix(count, n, seed):
    """float32 (count, n): a few distinct values in long runs of equals, with NaN (two payloads), both zeros, both
    infinities, the largest and the smallest numbers scattered in"""
    rng = np.random.default_rng(seed)
    pool = np.array([0.5, 0.5, 0.25, -0.25, 1.0, -1.0, 0.0, -0.0, np.inf, -np.inf, 3.4028235e38, 1e-45, -1e-45, np.nan],
                    dtype=np.float32)
    matrix = rng.choice(pool, size=(count, n))
    ordinary = rng.random((count, n)) < 0.3
    matrix[ordinary] = rng.uniform(-1, 1, size=int(ordinary.sum())).astype(np.float32)
    bits = matrix.view(np.uint32)
    odd = np.isnan(matrix) & (rng.random((count, n)) < 0.5)
    bits[odd] = 0xFFC12345   # (a negative NaN with a payload: the one NaN key all the same)
    return matrix


def marks_over(matrix, seed, base=0):
    """(thresholds float32 (Q,), marks int64 (Q,)) cycling through the kinds of mark: the value and position of a column
    (a rank), the value of a column with position -1 / INT64_MAX / just before / just behind / far from it, a NaN
    threshold, a threshold that no column holds"""
    rng = np.random.default_rng(seed)
    count, n = matrix.shape
    thresholds = np.zeros(count, dtype=np.float32)
    marks = np.zeros(count, dtype=np.int64)
    for q in range(count):
        column = int(rng.integers(0, n))
        thresholds[q] = matrix[q, column]
        kind = q % 8
        marks[q] = (base + column, -1, INT64_MAX, base + column - 1, base + column + 1, base + int(rng.integers(0, n)),
                    base + column, base + n + 5)[kind]
        if kind == 6:
            thresholds[q] = np.float32(np.nan)
        if kind == 7:
            thresholds[q] = np.float32(0.3)
    return thresholds, marks
