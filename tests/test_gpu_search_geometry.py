"""The reduction kernels of the sliced searches alone at their widest launch geometry, where the feature files do not reach:
topk_select / topk_select_excluding / topk_merge with a segment length rounded up to the unroll step, with exactly
MAX_SEGMENTS lists per row (16 384 entries through topk_merge's loop at k = 64), with the next length up and with a last
segment of one column; rank_fold's strided loop over more than 64 and more than 128 partial counts per row; exclusion lists
of rank_fold of 1 and of 64 entries on both sides of FOLD_WAVES rows. Host-built float32 matrices through the dense entry
points, against topk_by_the_contract and ranks_by_the_contract in numpy: values as bits, positions and counts equal. Every
test asserts, through the workspace size the library asks for, the geometry it claims to reach."""
import numpy as np
import pytest

from query_topk_reference import rows_of_every_kind, same_topk, topk_by_the_contract
from ranks_reference import hostile_matrix, marks_over, ranks_by_the_contract
from test_gpu_analogies import dense_topk_excluding
from test_gpu_query_topk import dense_topk, memb
from test_gpu_ranks import BLOCK_RUN, dense_ranks, ranks

pytestmark = pytest.mark.gpu

# memb_query_topk's plan (hip_query_topk.h, planTopkSegments) for at most 32 rows: a row is cut into at most MAX_SEGMENTS
# segments of at least MIN_SEGMENT columns, the length rounded up to BATCH * UNROLL
MIN_SEGMENT, STEP, MAX_SEGMENTS = 1024, 64 * 4, 256
BASE = 1000
# n: (segments, segment length) as the plan must come out
WIDE = {
    256 * 1024 + 1: (205, 1280),    # the length 1025 rounded up to 1280: fewer than 256 segments, the last of 1025 columns
    256 * 1280: (256, 1280),        # MAX_SEGMENTS full segments
    256 * 1280 + 1: (214, 1536),    # the next length up, the last segment of 513 columns
}
WIDTH = 64                          # of an exclusion list: one lane per entry


def assert_plan(count, n, k, segments, length):
    """the plan the test was written for is the library's: the lists it asks room for are `segments` per row, which of
    the multiples of STEP only `length` gives"""
    assert memb().QUERY_TOPK_MIN_SEGMENT == MIN_SEGMENT
    assert length % STEP == 0 and length >= MIN_SEGMENT and -(-n // length) == segments <= MAX_SEGMENTS
    assert length - STEP < max(MIN_SEGMENT, -(-n // MAX_SEGMENTS))   # (the least such multiple)
    assert memb().dense_topk_workspace_bytes(count, n, k) == count * segments * k * 8, (count, n, k)


def exclusion_lists(best, n, segments, length):
    """int64 (rows, 64): twenty of each row's own best 64 (whichever segments they lie in), both ends of the first, of a
    middle and of the last segment, -1 behind them"""
    middle = segments // 2
    fixed = [0, length - 1, middle * length, middle * length + length - 1, (segments - 1) * length, n - 1]
    lists = np.full((best.shape[0], WIDTH), -1, dtype=np.int64)
    lists[:, :20] = best[:, 0:40:2]
    lists[:, 20:20 + len(fixed)] = BASE + np.array(fixed, dtype=np.int64)
    reached = {int(segment) for segment in (lists[lists >= 0] - BASE) // length}
    assert {0, middle, segments - 1} <= reached
    return lists


def topk_without(matrix, lists):
    """topk_by_the_contract at k = 64 over each row without the columns its list names, the positions mapped back"""
    values = np.empty((matrix.shape[0], 64), dtype=np.float32)
    positions = np.empty((matrix.shape[0], 64), dtype=np.int64)
    for q in range(matrix.shape[0]):
        named = lists[q][lists[q] >= 0] - BASE
        kept = np.setdiff1d(np.arange(matrix.shape[1]), named)
        got = topk_by_the_contract(matrix[q:q + 1, kept], 64)
        assert (got[1] >= 0).all()
        values[q], positions[q] = got[0][0], BASE + kept[got[1][0]]
    return values, positions


def cut(want, rows, k):
    """rows `rows` of a reference worked out at k = 64, cut to k: topk_by_the_contract cuts one order to k"""
    return np.ascontiguousarray(want[0][rows, :k]), np.ascontiguousarray(want[1][rows, :k])


def selection_case(n, segments, length, picked=None):
    named = rows_of_every_kind(n, seed=7)
    if picked is not None:
        named = [named[i] for i in picked]
    matrix = np.stack([row for _, row in named])
    plain = topk_by_the_contract(matrix, 64, base=BASE)
    lists = exclusion_lists(plain[1], n, segments, length)
    without = topk_without(matrix, lists)
    assert not np.array_equal(plain[1], without[1])
    return [name for name, _ in named], matrix, plain, lists, without


def check_selection(names, matrix, plain, lists, without, rows, k, ld):
    rows = list(rows)
    got = dense_topk(matrix[rows], k, ld=ld, base=BASE)
    assert same_topk(got, cut(plain, rows, k)), ('plain', [names[q] for q in rows], k, ld)
    got = dense_topk_excluding(matrix[rows], k, lists[rows], ld=ld, base=BASE)
    assert same_topk(got, cut(without, rows, k)), ('excluding', [names[q] for q in rows], k, ld)


# ---- 1. the selection ----

@pytest.mark.parametrize('n', sorted(WIDE))
def test_selection_at_the_widest_plans(native, n):
    segments, length = WIDE[n]
    names, matrix, plain, lists, without = selection_case(n, segments, length)
    kinds = len(names)
    for c, (k, ld) in enumerate(((1, n), (1, n + 3), (64, n), (64, n + 3))):
        for count in (1, 3):
            assert_plan(count, n, k, segments, length)
        # every kind of row alone and among three over the four combinations
        check_selection(names, matrix, plain, lists, without, [c], k, ld)
        check_selection(names, matrix, plain, lists, without, [c + 4], k, ld)
        check_selection(names, matrix, plain, lists, without, [(2 * c + i) % kinds for i in range(3)], k, ld)
    if segments == MAX_SEGMENTS:
        assert segments * 64 == 16384   # (the entries of one row through topk_merge at k = 64)


def test_selection_of_five_rows_and_a_last_segment_of_one_column(native):
    n, segments, length = 3 * MIN_SEGMENT + 1, 4, MIN_SEGMENT
    assert n - (segments - 1) * length == 1
    # ascending: the best column is the last segment's one; constant: it comes last among equals
    names, matrix, plain, lists, without = selection_case(n, segments, length, picked=(0, 2, 4, 5, 7))
    assert names[0] == 'ascending' and plain[1][0, 0] == BASE + n - 1 and len(names) == 5   # (no multiple of WAVES_PER_BLOCK)
    for k in (1, 64):
        assert_plan(5, n, k, segments, length)
        for ld in (n, n + 3):
            check_selection(names, matrix, plain, lists, without, range(5), k, ld)


# ---- 2. the ranks ----

@pytest.mark.parametrize('n,blocks', [(64 * BLOCK_RUN + 1, 65), (130 * BLOCK_RUN - 5, 130)])
def test_rank_fold_goes_round_its_partial_counts(native, n, blocks):
    """more partial counts per row than rank_fold's wavefront has lanes: two passes with one count in the second, three
    with a ragged last one"""
    assert BLOCK_RUN == 2048 and -(-n // BLOCK_RUN) == blocks and blocks > 64 and blocks % 64 != 0
    assert ranks().dense_ranks_workspace_bytes(2, n) == (2 * blocks * 4 + 7) // 8 * 8
    tile = hostile_matrix(2, 4099, seed=71)
    matrix = np.ascontiguousarray(np.tile(tile, (1, -(-n // 4099)))[:, :n])
    matrix[:, n - 1] = np.nan   # (precedes every mark but a NaN one: the one column of block 64 counts)
    thresholds, marks = marks_over(matrix, seed=n)
    want = ranks_by_the_contract(matrix, thresholds, marks)
    # the partial counts of the last pass are not zero: a loop that stopped before it would show
    last_pass = (blocks - 1) // 64 * 64 * BLOCK_RUN
    assert (ranks_by_the_contract(matrix[:, last_pass:], thresholds, marks, last_pass) > 0).all()
    assert dense_ranks(matrix, thresholds, marks).tolist() == want.tolist()


def test_rank_lists_of_one_and_sixty_four_entries(native):
    n = 5003
    matrix = hostile_matrix(8, n, seed=72)
    thresholds, marks = marks_over(matrix, seed=73)
    plain = ranks_by_the_contract(matrix, thresholds, marks)
    rng = np.random.default_rng(74)
    one = rng.integers(0, n, size=(8, 1)).astype(np.int64)
    wide = rng.integers(0, n, size=(8, WIDTH)).astype(np.int64)
    wide[:, 31] = wide[:, 62] = wide[:, 0]            # a repeat whose first occurrence is lane 0
    wide[:, 40:44] = -1                               # padding
    wide[:, 44], wide[:, 45] = n, n + 5               # beyond the last column
    wide[:, 46], wide[:, 47] = -7, -(1 << 62)         # before the first
    wide[:, 7] = np.clip(marks, -1, n)                # the mark itself
    # lane 63: a column no other lane names and that precedes the mark wherever the row has one
    for q in range(8):
        counted = [c for c in np.argsort(-np.nan_to_num(matrix[q], nan=np.inf), kind='stable')[:80] if c not in wide[q, :63]]
        wide[q, 63] = counted[0]
    turned = np.ascontiguousarray(wide[:, ::-1])      # the same sets: the repeat's last occurrence in lane 63
    wants = [(lists, ranks_by_the_contract(matrix, thresholds, marks, 0, lists)) for lists in (one, wide, turned)]
    assert wants[1][1].tolist() == wants[2][1].tolist() and (wants[1][1] < plain).any() and (wants[0][1] <= plain).all()
    alone = wide.copy()
    alone[:, :63] = -1                                # only lane 63 names a column
    wants.append((alone, ranks_by_the_contract(matrix, thresholds, marks, 0, alone)))
    assert (wants[3][1] < plain).any()
    for count in (4, 5, 8):                           # rank_fold: one block of FOLD_WAVES rows, one more row, two blocks
        for lists, want in wants:
            assert lists.shape[1] in (1, WIDTH)
            got = dense_ranks(matrix[:count], thresholds[:count], marks[:count], lists=np.ascontiguousarray(lists[:count]))
            assert got.tolist() == want[:count].tolist(), (count, lists.shape[1])
