"""The contract of include/memb_hip_pairs.h restated in numpy, for the pair tests on both sides (tests/test_pairs_host.py,
tests/test_gpu_pairs.py). Every product, sum, root and quotient below is ONE IEEE float32 operation of numpy's: arrays and
scalars of numpy.float32 never pass through float64 and are never fused.

    piece products d_k = ((x0 y0 + x1 y1) + x2 y2) + x3 y3 over the columns 4k .. 4k + 3, a column >= dim is +0.0
    lane partials  p_l = d_l + d_(l + 64) + ..  in ascending k, starting from d_l; +0.0 where lane l has no piece. A lane
                   with piece l and no piece l + 64 keeps d_l's bits (which may be -0.0): selected, not added to +0.0
    butterfly      stride 1, 2, 4, 8, 16, 32: p_l = p_l + p_(l xor stride), all 64 at once; dot = p_0
    norms          na, nb: norms_reference's, of x and of y
    cosine         dot / ((na < 1e-12 ? 1e-12 : na) * (nb < 1e-12 ? 1e-12 : nb)), not clamped

pairs_by_the_contract works on whole matrices; pair_of_two_rows walks one pair with scalars, lane by lane, and is what the
matrix form is itself checked against."""
import numpy as np

from norms_reference import EPS, LANES, norm_of_one_row, norms_by_the_contract


def pair_of_two_rows(x, y):
    """(cosine, dot, na, nb) of one pair, the contract spelt out with numpy.float32 scalars only"""
    x = [np.float32(value) for value in x]
    y = [np.float32(value) for value in y]
    dim = len(x)
    assert len(y) == dim
    pieces = (dim + 3) // 4
    zero = np.float32(0.0)
    with np.errstate(all='ignore'):
        products = []
        for k in range(pieces):
            a = [x[4 * k + j] if 4 * k + j < dim else zero for j in range(4)]
            b = [y[4 * k + j] if 4 * k + j < dim else zero for j in range(4)]
            products.append(((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3])
        partial = []
        for lane in range(LANES):
            if lane >= pieces:
                partial.append(zero)
                continue
            p = products[lane]   # (kept as it is where the lane has no further piece: -0.0 stays -0.0)
            for k in range(lane + LANES, pieces, LANES):
                p = p + products[k]
            partial.append(p)
        for stride in (1, 2, 4, 8, 16, 32):
            partial = [partial[lane] + partial[lane ^ stride] for lane in range(LANES)]
        assert all(p.tobytes() == partial[0].tobytes() for p in partial)   # commutative: every lane holds the same bits
        dot = partial[0]
        na, nb = norm_of_one_row(x), norm_of_one_row(y)
        cosine = dot / ((EPS if na < EPS else na) * (EPS if nb < EPS else nb))
    assert all(value.dtype == np.float32 for value in (cosine, dot, na, nb))
    return cosine, dot, na, nb


def dots_by_the_contract(x, y):
    """float32 (n,) dots of the pairs (x[i], y[i]) of two float32 (n, dim) matrices"""
    x = np.ascontiguousarray(x, dtype=np.float32)
    y = np.ascontiguousarray(y, dtype=np.float32)
    assert x.shape == y.shape
    n, dim = x.shape
    pieces = (dim + 3) // 4
    columns = np.zeros((2, 4, n, pieces), dtype=np.float32)
    for side, values in enumerate((x, y)):
        for j in range(4):
            taken = values[:, j::4]
            columns[side, j, :, :taken.shape[1]] = taken
    with np.errstate(all='ignore'):
        sums = columns[0, 0] * columns[1, 0] + columns[0, 1] * columns[1, 1]
        sums = sums + columns[0, 2] * columns[1, 2]
        sums = sums + columns[0, 3] * columns[1, 3]
        partial = np.zeros((n, LANES), dtype=np.float32)
        for lane in range(min(LANES, pieces)):
            p = sums[:, lane].copy()
            for k in range(lane + LANES, pieces, LANES):
                p = p + sums[:, k]
            partial[:, lane] = p
        for stride in (1, 2, 4, 8, 16, 32):
            partial = partial + partial[:, np.arange(LANES) ^ stride]
        assert partial.dtype == np.float32
        return partial[:, 0].copy()


def pairs_by_the_contract(x, y):
    """(cosines (n,), dots (n,), norms (n, 2)) of the pairs (x[i], y[i]), all float32"""
    dots = dots_by_the_contract(x, y)
    norms = np.stack([norms_by_the_contract(x), norms_by_the_contract(y)], axis=1)
    floored = np.where(norms < EPS, EPS, norms).astype(np.float32)
    with np.errstate(all='ignore'):
        cosines = dots / (floored[:, 0] * floored[:, 1])
    assert cosines.dtype == np.float32 and norms.dtype == np.float32
    return cosines, dots, norms


def pairs_of_rows(values):
    """pairs_by_the_contract over an interleaved float32 (2n, dim) matrix: pair i is the rows 2i and 2i + 1"""
    values = np.ascontiguousarray(values, dtype=np.float32)
    return pairs_by_the_contract(values[0::2], values[1::2])
