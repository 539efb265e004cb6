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
