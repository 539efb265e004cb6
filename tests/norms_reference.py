"""The contract of include/memb_hip_norms.h restated in numpy, for the norm tests on both sides (tests/test_norms_host.py,
tests/test_gpu_norms.py). Every product, sum, root and quotient below is ONE IEEE float32 operation of numpy's: arrays and
scalars of numpy.float32 never pass through float64 and are never fused.

    piece sums     q_k = ((v0 v0 + v1 v1) + v2 v2) + v3 v3 over the columns 4k .. 4k + 3, a column >= dim is +0.0
    lane partials  p_l = q_l + q_(l + 64) + ..  in ascending k, starting from q_l; +0.0 where lane l has no piece
    butterfly      stride 1, 2, 4, 8, 16, 32: p_l = p_l + p_(l xor stride), all 64 at once
    norm           sqrt(p_0)
    unit row       v_i / (norm < 1e-12 ? 1e-12 : norm)

norms_by_the_contract / unit_rows_by_the_contract work on whole matrices; norm_of_one_row walks one row with scalars, lane
by lane, and is what the matrix form is itself checked against."""
import os

import numpy as np

from conftest import bits_equal

LANES = 64
EPS = np.float32(1e-12)


def norm_of_one_row(row):
    """the contract spelt out for one row, with numpy.float32 scalars only"""
    row = [np.float32(value) for value in row]
    dim = len(row)
    pieces = (dim + 3) // 4
    zero = np.float32(0.0)
    with np.errstate(all='ignore'):
        sums = []
        for k in range(pieces):
            v = [row[4 * k + j] if 4 * k + j < dim else zero for j in range(4)]
            sums.append(((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]) + v[3] * v[3])
        partial = []
        for lane in range(LANES):
            if lane >= pieces:
                partial.append(zero)
                continue
            p = sums[lane]
            for k in range(lane + LANES, pieces, LANES):
                p = p + sums[k]
            partial.append(p)
        for stride in (1, 2, 4, 8, 16, 32):
            partial = [partial[lane] + partial[lane ^ stride] for lane in range(LANES)]
        assert all(p.tobytes() == partial[0].tobytes() for p in partial)   # commutative: every lane holds the same bits
        return np.sqrt(partial[0])


def norms_by_the_contract(values):
    """float32 (n,) norms of the rows of a float32 (n, dim) matrix"""
    values = np.ascontiguousarray(values, dtype=np.float32)
    n, dim = values.shape
    pieces = (dim + 3) // 4
    columns = np.zeros((4, n, pieces), dtype=np.float32)
    for j in range(4):
        taken = values[:, j::4]
        columns[j, :, :taken.shape[1]] = taken
    with np.errstate(all='ignore'):
        sums = columns[0] * columns[0] + columns[1] * columns[1]
        sums = sums + columns[2] * columns[2]
        sums = sums + columns[3] * columns[3]
        partial = np.zeros((n, LANES), dtype=np.float32)
        for lane in range(min(LANES, pieces)):
            p = sums[:, lane].copy()
            for k in range(lane + LANES, pieces, LANES):
                p = p + sums[:, k]
            partial[:, lane] = p
        for stride in (1, 2, 4, 8, 16, 32):
            partial = partial + partial[:, np.arange(LANES) ^ stride]
        assert partial.dtype == np.float32
        return np.sqrt(partial[:, 0])


def unit_rows_by_the_contract(values, norms=None):
    """(unit rows, norms): every element divided by its row's max(norm, 1e-12), one float32 division"""
    values = np.ascontiguousarray(values, dtype=np.float32)
    if norms is None:
        norms = norms_by_the_contract(values)
    divisor = np.where(norms < EPS, EPS, norms).astype(np.float32)
    with np.errstate(all='ignore'):
        unit = values / divisor[:, None]
    assert unit.dtype == np.float32
    return unit, norms


def ids_with_misses(count, n_rows, seed, repeated=True):
    """`count` row ids below n_rows in no particular order, some repeated, with 0xFFFFFFFF and ids >= n_rows among them"""
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n_rows, size=count, dtype=np.int64)
    if repeated and count > 4:
        rows[count // 2] = rows[0]
        rows[count // 3] = rows[0]
    rows[3::11] = 0xFFFFFFFF
    rows[5::17] = n_rows + (seed % 7)
    return rows.astype(np.uint32)


# ---- special rows, built with the public Builder ----

def special_model(native, directory, dim=300):
    """a `full` model (it holds the floats it is given): rows of 2^-70, a row of +0.0, a row of -0.0, a row of mixed tiny
    values, an ordinary row"""
    rng = np.random.default_rng(70)
    vectors = np.zeros((6, dim), dtype=np.float32)
    vectors[0] = np.float32(2.0 ** -70)
    vectors[1] = -np.float32(2.0 ** -70)
    vectors[2] = 0.0
    vectors[3] = -0.0
    vectors[4] = (rng.integers(-9, 10, size=dim) * 2.0 ** -72).astype(np.float32)
    vectors[5] = rng.standard_normal(dim).astype(np.float32)
    builder = native.Builder(dim, 'full', 8)
    builder.add_words(['s{}'.format(i) for i in range(len(vectors))], vectors)
    path = os.path.join(str(directory), 'special_{}.bin'.format(dim))
    builder.save(path)
    return path, vectors


def check_special_rows(vectors, norms, unit):
    """what the special model's rows 0 .. 5 must give, whoever computed them"""
    want_unit, want_norms = unit_rows_by_the_contract(vectors)
    assert bits_equal(norms, want_norms) and bits_equal(unit, want_unit)
    # 300 squares of 2^-70 sum to 300 * 2^-140, below the smallest normal float32 (2^-126): a flush would give 0
    total = np.float32(300 * 2.0 ** -140)
    assert 0 < total < np.float32(1.1754944e-38)
    assert norms[0] == np.sqrt(total) and norms[0] > 0 and norms[1] == norms[0]
    # below eps: divided by 1e-12, not by the norm
    assert bits_equal(unit[0], vectors[0] / np.float32(1e-12)) and (unit[1] < 0).all()
    # zero rows stay what they are, signs kept
    assert norms[2] == 0 and norms[3] == 0 and not np.signbit(norms[2:4]).any()
    assert not unit[2].any() and not np.signbit(unit[2]).any()
    assert not unit[3].any() and np.signbit(unit[3]).all()
    assert abs(float(np.sqrt((unit[5].astype(np.float64) ** 2).sum())) - 1.0) < 1e-6
