"""The pooling contracts restated in numpy, for every tests/test_*pooled*.py: the sequential order of
include/memb_hip_pooled.h / memb_hip_pooled_known.h, the chunked order of include/memb_hip_pooled_chunked.h (every function
of it takes the chunk length C from the caller, who reads memb_amd.POOL_CHUNK), the merge of a ReadersUnion's rows
(include/memb_hip_pooled_union.h), and the id and batch builders those tests share. Pure numpy: no torch, no GPU.

Offsets are read as the kernels read them: uint32, clamped to n, a backwards range empty -- so bags may overlap."""
import numpy as np

from conftest import bits_equal

UNKNOWN = 0xFFFFFFFF


def offsets_of(lengths, first=0):
    return (first + np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])).astype(np.int64)


def clamped(offsets, n):
    return np.minimum(np.asarray(offsets).astype(np.int64) & 0xFFFFFFFF, n)


# ---- the sequential order ----

def compacted(rows, offsets, n_rows):
    """The batch without its unknown entries (row id >= n_rows): (rows, offsets, positions of the kept entries in `rows`).
    Bags may overlap: each is gathered."""
    rows = np.asarray(rows, dtype=np.uint32)
    bounds = clamped(offsets, len(rows))
    kept = []
    lengths = []
    for begin, end in zip(bounds[:-1], bounds[1:]):
        positions = np.arange(begin, max(begin, end))
        positions = positions[rows[positions] < n_rows]
        kept.append(positions)
        lengths.append(len(positions))
    positions = np.concatenate(kept).astype(np.int64) if kept else np.zeros(0, dtype=np.int64)
    return rows[positions], offsets_of(lengths), positions


def sequential_by_the_contract(values, rows, offsets, n_rows, mode, skip):
    """THE loop of include/memb_hip_pooled.h and, with skip, of memb_hip_pooled_known.h. values: the (n, dim) float32 rows of
    the entries (zeros for an unknown one). Per bag, over its entries in entry order -- with skip over K, its KNOWN entries
    (rows[i] < n_rows) only, an unknown one adding nothing, not even +0.0 --: acc = v_first, then acc = acc + v_i, one
    float32 addition each; 'mean': one float32 division by float32(count) at the end; +0.0 for a bag without an entry
    (with skip: without a known one). Returns (vectors, counts): counts the bags' known entries with skip, their entries
    without. `rows` and `n_rows` are read with skip only.

    The loop runs for all bags side by side: step j adds entry j of every bag that has one."""
    n, dim = values.shape
    if skip:
        _, dense, positions = compacted(rows, offsets, n_rows)
        begin, length = dense[:-1], dense[1:] - dense[:-1]
    else:
        bounds = clamped(offsets, n)
        begin, length = bounds[:-1], np.maximum(bounds[1:] - bounds[:-1], 0)
    out = np.zeros((len(begin), dim), dtype=np.float32)
    for step in range(int(length.max()) if len(length) else 0):
        active = np.nonzero(length > step)[0]
        entries = begin[active] + step
        addend = values[positions[entries] if skip else entries]
        out[active] = addend if step == 0 else np.add(out[active], addend, dtype=np.float32)
    if mode == 'mean':
        filled = length > 0
        out[filled] = np.divide(out[filled], length[filled].astype(np.float32)[:, None], dtype=np.float32)
    return out, length.astype(np.uint32)


def pooled_by_the_contract(values, offsets, mode):
    """The plain case: every entry counts (a missing row is its +0.0 row), vectors only."""
    return sequential_by_the_contract(values, None, offsets, None, mode, False)[0]


def ids_with_misses(count, n_rows, seed):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n_rows, size=count, dtype=np.int64)
    if count:
        rows[::7] = 0xFFFFFFFF
        rows[3::11] = n_rows + 5
        rows[0] = n_rows
        rows[-1] = 0xFFFFFFFF
    return rows.astype(np.uint32)


def ids_with_unknowns(count, n_rows, seed, share=0.3):
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n_rows, size=count, dtype=np.int64)
    unknown = rng.random(count) < share
    rows[unknown] = rng.choice([UNKNOWN, n_rows, n_rows + 5, 0xFFFFFFFE], size=int(unknown.sum()))
    return rows.astype(np.uint32)


# ---- a ReadersUnion's rows ----

def merged_rows(mode, pieces):
    """The union's rows by the explicit order: (((v1 + v2) + v3) ..) / R, or the readers' rows side by side"""
    if mode == 'concatenate':
        return np.hstack(pieces)
    total = pieces[0]
    for piece in pieces[1:]:
        total = np.add(total, piece, dtype=np.float32)
    return np.divide(total, np.float32(len(pieces)), dtype=np.float32)


def union_ids(count, readers, seed, n_rows):
    """Row ids drawn independently per reader -- an entry is missing in one reader, in another, in all or in none -- and a
    stretch of entries that no reader has"""
    rows = [ids_with_misses(count, n_rows, seed + 100 * position) for position in range(readers)]
    for ids in rows:
        ids[count // 2:count // 2 + 9] = 0xFFFFFFFF
    return rows


# ---- the chunked order ----

def contract_lengths(chunk):
    return [0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk, 2 * chunk + 1, 0, 5 * chunk + 3, 3, 40 * chunk + 5, 1]


LONGEST = 10   # the bag of 40 C + 5 entries among contract_lengths


def contract_batch(chunk, n_rows, seed):
    """(rows, offsets): the bags of contract_lengths in one batch whose first bag begins at entry 3, so that no chunk starts
    on a tile boundary; random rows with repeats, every 7th entry 0xFFFFFFFF, one entry n_rows + 5."""
    offsets = offsets_of(contract_lengths(chunk), first=3)
    rng = np.random.default_rng(seed)
    rows = rng.integers(0, n_rows, size=int(offsets[-1])).astype(np.uint32)
    rows[100:140] = rows[60:100]   # repeats
    rows[::7] = UNKNOWN
    rows[int(offsets[LONGEST]) + chunk + 2] = n_rows + 5
    return rows, offsets


def inner_batches(chunk, n_rows, seed):
    """[(name, rows, offsets)]: bags that cover only the MIDDLE of their batch -- the first offset lies behind entry 0 and
    the last one well before n, so the entries behind the last bag belong to no bag. One batch ends in a long bag, one in
    a bag of at most C entries, one is a single short bag (n = 10, offsets [0, 4]: every chunk slot but one is spare)."""
    rng = np.random.default_rng(seed)
    batches = []
    for name, lengths, slack in (('long last bag', [3, chunk + 1, 0, 7 * chunk + 9], 5 * chunk + 3),
                                 ('short last bag', [2 * chunk + 5, chunk, 0, chunk - 3], 9 * chunk + 1),
                                 ('one short bag', [4], 6)):
        first = 0 if name == 'one short bag' else 5
        offsets = offsets_of(lengths, first=first)
        rows = rng.integers(0, n_rows, size=int(offsets[-1]) + slack).astype(np.uint32)
        rows[::7] = UNKNOWN
        rows[-1] = 1   # (known entries behind the last bag: they must not be counted)
        batches.append((name, rows, offsets))
    return batches


def derived_offsets(offsets, n, chunk):
    """(derived, first): one bag per chunk -- bag b has max(1, ceil(L / C)) of them, chunk j beginning at begin + C j -- and
    first[b], the first chunk of bag b (first[bags]: all chunks). For ascending offsets."""
    bounds = clamped(offsets, n)
    derived, first = [], [0]
    for begin, end in zip(bounds[:-1], bounds[1:]):
        chunks = max(1, -(-(int(end) - int(begin)) // chunk))
        derived.extend(int(begin) + chunk * j for j in range(chunks))
        first.append(first[-1] + chunks)
    derived.append(int(bounds[-1]))
    return np.array(derived, dtype=np.int64), np.array(first, dtype=np.int64)


def in_order(vectors):
    """acc = v_0, acc = acc + v_i: one float32 addition each. None for no vectors."""
    acc = None
    for vector in vectors:
        acc = vector.copy() if acc is None else np.add(acc, vector, dtype=np.float32)
    return acc


def finish(total, count, mode, dim):
    if total is None:
        return np.zeros(dim, dtype=np.float32)
    if mode == 'mean' and count:
        return np.divide(total, np.float32(count), dtype=np.float32)
    return total


def chunked_by_the_contract(values, rows, offsets, n_rows, mode, skip, chunk):
    """values: the (n, dim) float32 rows of the entries (zeros for an unknown one). Returns (vectors, counts): counts the
    bags' known entries with skip, their entries without."""
    rows = np.asarray(rows, dtype=np.uint32)
    bounds = clamped(offsets, len(rows))
    dim = values.shape[1]
    out = np.zeros((len(bounds) - 1, dim), dtype=np.float32)
    counts = np.zeros(len(bounds) - 1, dtype=np.uint32)
    for bag, (begin, end) in enumerate(zip(bounds[:-1], bounds[1:])):
        partial = []
        for low in range(int(begin), int(end), chunk):
            positions = np.arange(low, min(int(end), low + chunk))
            if skip:
                positions = positions[rows[positions] < n_rows]
            counts[bag] += len(positions)
            if len(positions):
                partial.append(in_order(values[positions]))   # a chunk without a known entry contributes nothing
        out[bag] = finish(in_order(partial), counts[bag], mode, dim)
    return out, counts


def from_partial_sums(partial, chunk_counts, first, mode, counts, dim):
    """The in-order loop over the chunks' partial sums (partial[k]: chunk k, chunk_counts[k]: the entries that went into it
    -- a chunk with none is left out); counts: what 'mean' divides bag b by."""
    out = np.zeros((len(first) - 1, dim), dtype=np.float32)
    for bag in range(len(first) - 1):
        used = [partial[k] for k in range(first[bag], first[bag + 1]) if chunk_counts[k]]
        out[bag] = finish(in_order(used), counts[bag], mode, dim)
    return out


def chunked_side_by_side(values, rows, offsets, n_rows, mode, skip, chunk):
    """chunked_by_the_contract for batches of very many bags, the same bits (tests/test_pooled_chunked_host.py proves it):
    a bag of at most C entries is one chunk, so its result is the in-order loop over its entries -- the known ones with
    skip -- and that loop runs for all such bags side by side, step j adding entry j of every bag that has one. Longer bags
    go through chunked_by_the_contract one by one."""
    rows = np.asarray(rows, dtype=np.uint32)
    bounds = clamped(offsets, len(rows))
    begin, end = bounds[:-1], bounds[1:]
    length = np.maximum(end - begin, 0)
    dim = values.shape[1]
    out = np.zeros((len(begin), dim), dtype=np.float32)
    if skip:   # entry j of a bag: the j-th known position at or behind its begin
        known = rows < n_rows
        before = np.concatenate([[0], np.cumsum(known)]).astype(np.int64)
        positions = np.nonzero(known)[0]
        start = before[begin]
        counts = np.where(length > 0, before[np.maximum(end, begin)] - start, 0)
    else:
        positions = np.arange(len(rows), dtype=np.int64)
        start = begin
        counts = length
    short = length <= chunk
    steps = counts[short]
    for step in range(int(steps.max()) if len(steps) else 0):
        active = np.nonzero(short & (counts > step))[0]
        addend = values[positions[start[active] + step]]
        out[active] = addend if step == 0 else np.add(out[active], addend, dtype=np.float32)
    if mode == 'mean':
        filled = short & (counts > 0)
        out[filled] = np.divide(out[filled], counts[filled].astype(np.float32)[:, None], dtype=np.float32)
    for bag in np.nonzero(~short)[0]:
        out[bag] = chunked_by_the_contract(values, rows, bounds[bag:bag + 2], n_rows, mode, skip, chunk)[0][0]
    return out, counts.astype(np.uint32)


# ---- batches for tests/test_gpu_pooled_chunked_geometry.py and the host tests of the same edges ----

# memb_amd/csrc/hip_pooled_chunked.h: PLAN_THREADS = 256 threads scan PLAN_BAGS_PER_THREAD = 8 consecutive bags each, so a
# block of the plan owns PLAN_BAGS_PER_BLOCK = 2048 bags, and chunk_scan_sums scans PLAN_THREADS block sums per round
# (tests/test_pooled_chunked_host.py reads the header and asserts these three)
PLAN_THREADS = 256
PLAN_BAGS_PER_THREAD = 8
PLAN_BAGS_PER_BLOCK = PLAN_THREADS * PLAN_BAGS_PER_THREAD

PLAN_BAG_COUNTS = ([1, 7, 8, 9] + [blocks * PLAN_BAGS_PER_BLOCK + k for blocks in (1, 2) for k in (-1, 0, 1)]
                   + [3 * PLAN_BAGS_PER_BLOCK + k for k in range(1, PLAN_BAGS_PER_THREAD + 1)])


def ids_every_7th_unknown(count, n_rows, rng):
    rows = rng.integers(0, n_rows, size=count).astype(np.uint32)
    rows[::7] = UNKNOWN
    return rows


def plan_batch(chunk, bags, n_rows, seed):
    """(rows, offsets): `bags` bags of mostly 0 / 1 / 2 entries; bags of 2 C + 1 and 9 C entries, in turn, at the first and
    last bag and on both sides of every edge of a block of the plan. Random ids, every 7th unknown."""
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 3, size=bags)
    edges = {0, bags - 1}
    for block in range(PLAN_BAGS_PER_BLOCK, bags + 1, PLAN_BAGS_PER_BLOCK):
        edges |= {block - 1, block}
    for turn, bag in enumerate(sorted(edge for edge in edges if 0 <= edge < bags)):
        lengths[bag] = (2 * chunk + 1, 9 * chunk)[turn % 2]
    return ids_every_7th_unknown(int(lengths.sum()), n_rows, rng), offsets_of(lengths)


def second_round_batch(chunk, n_rows, seed):
    """(rows, offsets, long): more blocks of the plan than chunk_scan_sums scans in one round -- PLAN_THREADS blocks and one
    more and 3 bags -- of 0 / 1 / 2 entries, with six bags of 5 C + 3 entries (`long`) at the first bag, on both sides of
    the first block's edge and of the first round's, and at the last bag."""
    bags = PLAN_THREADS * PLAN_BAGS_PER_BLOCK + PLAN_BAGS_PER_BLOCK + 3
    rng = np.random.default_rng(seed)
    lengths = rng.integers(0, 3, size=bags)
    long = np.array([0, PLAN_BAGS_PER_BLOCK - 1, PLAN_BAGS_PER_BLOCK, PLAN_THREADS * PLAN_BAGS_PER_BLOCK - 1,
                     PLAN_THREADS * PLAN_BAGS_PER_BLOCK, bags - 1])
    lengths[long] = 5 * chunk + 3
    return ids_every_7th_unknown(int(lengths.sum()), n_rows, rng), offsets_of(lengths), long


def sub_batch(rows, offsets, picked):
    """(rows, offsets): the bags `picked` of a batch with ascending offsets, as a batch of their own."""
    rows = np.asarray(rows, dtype=np.uint32)
    lengths = [int(offsets[bag + 1] - offsets[bag]) for bag in picked]
    parts = [rows[int(offsets[bag]):int(offsets[bag + 1])] for bag in picked]
    return (np.concatenate(parts) if parts else np.zeros(0, dtype=np.uint32)), offsets_of(lengths)


EDGE_CHUNK_COUNTS = list(range(1, 21)) + [24, 25, 32, 33]   # around the 8-chunk batches of pool_chunks, both branches


def edge_lengths(chunk):
    """Bags of exactly j chunks, j over EDGE_CHUNK_COUNTS: (j - 1) C + r with r cycling over 1, C - 1 and C."""
    return [(j - 1) * chunk + (1, chunk - 1, chunk)[turn % 3] for turn, j in enumerate(EDGE_CHUNK_COUNTS)]


def edge_batch(chunk, n_rows, seed, reverse=False):
    """(rows, offsets): the bags of edge_lengths in one batch that begins at entry 3, as contract_batch does (reverse: the
    longest bag first -- another batch of the same n and bags). Random ids, every 7th unknown."""
    lengths = edge_lengths(chunk)
    offsets = offsets_of(lengths[::-1] if reverse else lengths, first=3)
    return ids_every_7th_unknown(int(offsets[-1]), n_rows, np.random.default_rng(seed)), offsets


UNKNOWN_CHUNKS = ('chunk 0', 'chunks 0..7', 'chunks 0..8', 'chunk 7', 'chunk 8', 'the last chunk', 'all but the last chunk',
                  'all but chunk 8', 'all chunks')


def with_unknown_chunks(rows, offsets, chunk, which):
    """`rows` with whole chunks of every bag made unknown (0xFFFFFFFF); `which`: one of UNKNOWN_CHUNKS. A bag that has no
    chunk of that index is left as it is."""
    rows = np.array(rows, dtype=np.uint32)
    for begin, end in zip(offsets[:-1], offsets[1:]):
        begin, end = int(begin), int(end)
        chunks = -(-(end - begin) // chunk)
        unknown = {'chunk 0': [0], 'chunks 0..7': range(8), 'chunks 0..8': range(9), 'chunk 7': [7], 'chunk 8': [8],
                   'the last chunk': [chunks - 1], 'all but the last chunk': range(chunks - 1),
                   'all but chunk 8': [j for j in range(chunks) if j != 8], 'all chunks': range(chunks)}[which]
        for j in unknown:
            if 0 <= j < chunks:
                rows[begin + chunk * j:min(end, begin + chunk * (j + 1))] = UNKNOWN
    return rows


def column_batch(chunk, n_rows, seed):
    """(rows, offsets): bags of 1, C, C + 1, 2 C + 1 and 9 C + 5 entries and an empty one, from entry 3."""
    offsets = offsets_of([1, chunk, 0, chunk + 1, 2 * chunk + 1, 9 * chunk + 5], first=3)
    return ids_every_7th_unknown(int(offsets[-1]), n_rows, np.random.default_rng(seed)), offsets


def wide_batch(chunk, n_rows, seed):
    """(rows, offsets): a dozen bags for rows of thousands of values, one of 2 C + 1 entries."""
    offsets = offsets_of([1, 0, 3, 9, 2, 17, 1, 2 * chunk + 1, 0, 5, 1, 2])
    return ids_every_7th_unknown(int(offsets[-1]), n_rows, np.random.default_rng(seed)), offsets


COLUMN_DIMS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 516, 1030]
COLUMN_STORAGES = [('trained', 4), ('uniform', 8), ('full', 8)]
COLUMN_ROWS = 300
WIDE_MODELS = [('trained', 8, 4096, 120), ('trained', 8, 9000, 40), ('trained', 4, 20000, 30), ('uniform', 8, 5001, 40),
               ('full', 8, 5001, 40)]   # (storage, bits, dim, rows): the very wide models of tests/test_gpu_pooled.py


def reversed_batch(rows, offsets):
    """(rows, offsets): the same n and the same number of bags, the bags' lengths and the entries in reverse order --
    another plan, other chunk counts per slot of the workspace."""
    lengths = (np.asarray(offsets[1:]) - np.asarray(offsets[:-1]))[::-1]
    return np.ascontiguousarray(np.asarray(rows, dtype=np.uint32)[::-1]), offsets_of(lengths, first=int(offsets[0]))


# ---- signed zeros under the chunked order: a model, its batches and what they must show ----

def signed_zero_model(native, directory):
    """A `full` model whose row 0 is all -0.0 and whose rows 1 and 2 are subnormal with mixed signs, -0.0 in their first
    columns."""
    rng = np.random.default_rng(41)
    count, dim = 40, 300
    vectors = rng.integers(-70000, 70000, size=(count, dim)).astype(np.float32) * np.float32(1.4e-45)
    vectors[0] = -0.0
    vectors[1, :50] = -0.0
    vectors[2, :30] = -0.0
    assert (np.abs(vectors) < 1.1754944e-38).all() and (vectors[1] > 0).any() and (vectors[1] < 0).any()
    builder = native.Builder(dim, 'full', 8)
    builder.add_words(['s{:04d}'.format(i) for i in range(count)], vectors)
    path = str(directory / 'signed_zero.bin')
    builder.save(path)
    return path, count


def skip_cases(chunk, count):
    """(rows, offsets): a bag of 3 C entries -- first chunk: one known row of -0.0 among unknown entries, middle chunk all
    0xFFFFFFFF, last chunk rows 0, 1, 2 and then row 0 again and again -- a bag of 2 C + 3 unknown entries, and a bag of
    3 C + 1 subnormal rows."""
    first = np.full(chunk, UNKNOWN, dtype=np.uint32)
    first[chunk // 2] = 0
    middle = np.full(chunk, UNKNOWN, dtype=np.uint32)
    last = np.zeros(chunk, dtype=np.uint32)
    last[:3] = [0, 1, 2]
    unknown = np.full(2 * chunk + 3, UNKNOWN, dtype=np.uint32)
    unknown[5] = count   # (an id that is not in the model is unknown too)
    subnormal = (np.arange(3 * chunk + 1) % (count - 1) + 1).astype(np.uint32)
    rows = np.concatenate([first, middle, last, unknown, subnormal])
    return rows, offsets_of([3 * chunk, len(unknown), len(subnormal)])


def check_skip_cases(result, counts, values, rows, offsets, count, chunk):
    """result, counts: mode='sum', missing='skip' of skip_cases; values: the entries' rows."""
    want, want_counts = chunked_by_the_contract(values, rows, offsets, count, 'sum', True, chunk)
    assert bits_equal(result, want) and np.array_equal(counts, want_counts)
    assert counts[0] == 1 + chunk and counts[1] == 0 and counts[2] == 3 * chunk + 1
    last = in_order(values[2 * chunk:3 * chunk])   # the last chunk's sum: -0.0 where rows 0, 1 and 2 all are
    negative_zero = (last == 0) & np.signbit(last)
    assert negative_zero[:30].all() and not negative_zero.all()
    # -0.0 (the first chunk) + nothing (the middle one) + last = last, -0.0 included; a +0.0 from the middle chunk or from
    # the first chunk's unknown entries would have turned those columns into +0.0
    assert bits_equal(result[0], last)
    assert not result[1].any() and not np.signbit(result[1]).any()   # no known entry: +0.0
    assert (result[2] != 0).any() and (np.abs(result[2]) < 1.1754944e-38).all()   # subnormal partial sums are kept


def signed_zero_rows(rows):
    """The known entries of `rows` as rows 0, 1 and 2 of signed_zero_model, whose first 30 columns are -0.0."""
    return np.where(rows == UNKNOWN, rows, rows % np.uint32(3)).astype(np.uint32)


def check_negative_zeros_survive(signed, holes, offsets, chunk):
    """(a reader of signed_zero_model, a batch of signed_zero_rows) by the contract, the first 30 columns of every bag with a
    known entry are -0.0, whichever chunks are unknown: one +0.0 added for an unknown chunk or entry would make them +0.0,
    and the reference would notice. Returns the contract's (sums, counts) with missing='skip'."""
    want, counts = chunked_by_the_contract(signed.rows_embedding(holes), holes, offsets, len(signed), 'sum', True, chunk)
    filled = counts > 0
    assert not want[:, :30].any() and np.signbit(want[filled, :30]).all() and not np.signbit(want[~filled]).any()
    assert not filled.any() or (want[filled, 50:] != 0).any()
    return want, counts
