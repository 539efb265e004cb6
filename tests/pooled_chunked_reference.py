"""The chunked order of include/memb_hip_pooled_chunked.h restated in numpy, for tests/test_pooled_chunked_host.py and
tests/test_gpu_pooled_chunked.py. Every function takes the chunk length C from the caller, who reads memb_amd.POOL_CHUNK.

Offsets are read as the kernels read them: uint32, clamped to n, a backwards range empty."""
import numpy as np

UNKNOWN = 0xFFFFFFFF


def offsets_of(lengths, first=0):
    return (first + np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])).astype(np.int64)


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


def clamped(offsets, n):
    return np.minimum(np.asarray(offsets).astype(np.int64) & 0xFFFFFFFF, n)


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


def sequential_by_the_contract(values, rows, offsets, n_rows, mode, skip):
    """The order of include/memb_hip_pooled.h / memb_hip_pooled_known.h: a bag's entries one after the other."""
    return chunked_by_the_contract(values, rows, offsets, n_rows, mode, skip, 1 << 40)


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
