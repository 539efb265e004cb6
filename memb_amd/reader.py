"""Read side: the reference's `memb.Reader` interface (python/memb/reader.py) over
the HIP batch-lookup path. `reader[word]` / `reader[list_of_words]` return numpy
float32 exactly as the reference does; words the model does not know give zeros.
Everything below "additions" is new: row ids, strided outputs, results that stay
on the GPU."""
import numbers
import threading
from abc import ABC, abstractmethod

import numpy as np

from . import _memb
from . import _memb_cosmul
from . import _memb_ranks
from . import _memb_within


class BaseReader(ABC):
    """What Reader, ReadersUnion and ShardedReader have in common: indexing and the
    exports built on batch_embedding."""

    def __getitem__(self, key):
        # a str selects one vector (1-D), a list a matrix (2-D); nothing else is accepted
        if isinstance(key, str):
            return self.word_embedding(key)
        if isinstance(key, list):
            return self.batch_embedding(key)
        raise TypeError('Key type is not supported')

    def to_keyed_vectors(self):
        """The whole model as a gensim KeyedVectors (one full-vocabulary lookup)"""
        try:
            from gensim.models import KeyedVectors
        except ImportError:
            raise ImportError('You must install gensim for KeyedVectors export')
        vocabulary = self.keys()
        exported = KeyedVectors(self.dim)
        exported.add(vocabulary, self.batch_embedding(vocabulary))
        return exported

    @abstractmethod
    def keys(self):
        pass

    @abstractmethod
    def word_embedding(self, word):
        pass

    @abstractmethod
    def batch_embedding(self, words):
        pass

    @abstractmethod
    def tokenizer_embedding(self, tokenzer):
        pass


def _current_stream(torch, index):
    '''torch's current stream on device `index` as a raw hipStream_t (the C call behind torch.cuda.current_stream,
    without building a Stream object: a microsecond per lookup)'''
    raw = getattr(torch._C, '_cuda_getCurrentRawStream', None)
    if raw is not None:
        try:
            return raw(index)
        except TypeError:   # (a private entry point: should its signature change, the public one still works)
            pass
    return torch.cuda.current_stream(index).cuda_stream


class WordBatches:
    """The word batches (packed query words: pinned + device buffers, kept between calls) of one Reader or ReadersUnion.
    A call takes a free batch, or a new one when every batch is out, and gives it back when it returns: no batch is ever
    shared by two calls in flight, and there are never more batches than concurrent callers. The free list is a stack,
    so a single caller keeps reusing one batch, whose next begin waits for the lookups still reading it."""

    def __init__(self):
        self._free = []
        self._lock = threading.Lock()
        self.last = None   # the batch given back most recently

    def take(self, device):
        with self._lock:
            if self._free:
                return self._free.pop()
        return _memb.WordBatch(device)

    def give(self, batch):
        with self._lock:
            self._free.append(batch)
            self.last = batch


def host_offsets(offsets):
    '''offsets of resolve_packed_device's host path as a contiguous numpy.uint32 array, never cast silently: any integer
    array or sequence; a value outside 0 .. 0xFFFFFFFF is a ValueError, anything but integers a TypeError. A
    C-contiguous uint32 array is passed on as it is.'''
    if isinstance(offsets, np.ndarray) and offsets.dtype == np.uint32 and offsets.flags.c_contiguous:
        return offsets
    array = np.asarray(offsets)
    if array.dtype.kind not in 'iu' and not isinstance(offsets, np.ndarray):
        # a sequence that numpy holds as float or object (Python ints beyond int64 among them): judged by its values
        values = list(offsets)
        if not all(isinstance(value, numbers.Integral) and not isinstance(value, (bool, np.bool_)) for value in values):
            raise TypeError('offsets must be integers')
        if min(values) < 0 or max(values) > 0xFFFFFFFF:
            raise ValueError('offsets must lie in 0 .. 0xFFFFFFFF')
        return np.array(values, dtype=np.uint32)
    if array.dtype.kind not in 'iu':
        raise TypeError('offsets must be integers, not {}'.format(array.dtype))
    if array.size and (array.min() < 0 or array.max() > 0xFFFFFFFF):
        raise ValueError('offsets must lie in 0 .. 0xFFFFFFFF')
    return np.ascontiguousarray(array, dtype=np.uint32)


POOL_MODES = {'sum': _memb.POOL_SUM, 'mean': _memb.POOL_MEAN}
BAGS_HOST_CHUNK = 1 << 16   # entries bags_embedding of a device='cpu' reader decodes at a time


def pool_mode(mode):
    """'sum' / 'mean' as the C ABI's MEMB_HIP_POOL_*; anything else (max pooling, weights) is not built"""
    if mode not in POOL_MODES:
        raise ValueError("pooling mode must be 'sum' or 'mean', not {!r}".format(mode))
    return POOL_MODES[mode]


POOL_MISSING = ('zero', 'skip')


def pool_missing(missing, return_counts):
    """missing='zero' (an entry that is not in the model is a row of +0.0 that counts) or 'skip' (it is left out of its bag
    and of the mean's count); counts exist for the skipping call only. Returns whether to skip."""
    if missing not in POOL_MISSING:
        raise ValueError("missing must be 'zero' or 'skip', not {!r}".format(missing))
    if return_counts and missing != 'skip':
        raise ValueError("return_counts needs missing='skip': counts are of the entries the model knows")
    return missing == 'skip'


POOL_REDUCTIONS = ('sequential', 'chunked')
POOL_CHUNK = _memb.POOL_CHUNK   # entries per chunk of reduction='chunked' (MEMB_HIP_POOL_CHUNK): a constant of the API


def pool_reduction(reduction):
    """reduction='sequential' (a bag's rows are added one after the other) or 'chunked' (a bag is cut into chunks of
    POOL_CHUNK entries whose sums are added in chunk order). Returns whether to chunk."""
    if reduction not in POOL_REDUCTIONS:
        raise ValueError("reduction must be 'sequential' or 'chunked', not {!r}".format(reduction))
    return reduction == 'chunked'


def chunk_offsets(offsets):
    """The chunks of reduction='chunked' as bags: (derived, first) for ascending int64 offsets -- derived the offsets of
    one bag per chunk (bag b: max(1, ceil(L / POOL_CHUNK)) of them), first[b] the first chunk of bag b, first[bags] all."""
    begins, lengths = offsets[:-1], offsets[1:] - offsets[:-1]
    per_bag = np.maximum(1, -(-lengths // POOL_CHUNK))
    first = np.concatenate(([0], np.cumsum(per_bag))).astype(np.int64)
    within = np.arange(first[-1], dtype=np.int64) - np.repeat(first[:-1], per_bag)
    derived = np.concatenate((np.repeat(begins, per_bag) + POOL_CHUNK * within, offsets[-1:])).astype(np.int64)
    return derived, first


def bag_offsets(offsets, n):
    """offsets of bags_embedding as a numpy.int64 array: bags + 1 integers, ascending, within 0 .. n. Anything else is a
    ValueError: on the host nothing is clamped silently."""
    array = np.asarray(offsets)
    if array.ndim != 1 or array.size < 1:
        raise ValueError('offsets needs bags + 1 entries')
    if array.dtype.kind not in 'iu':
        raise ValueError('offsets must be integers, not {}'.format(array.dtype))
    array = array.astype(np.int64) if array.dtype != np.uint64 else array
    if array.min() < 0 or array.max() > n:
        raise ValueError('offsets must lie in 0 .. len(rows) = {}'.format(n))
    array = array.astype(np.int64)
    if np.any(array[1:] < array[:-1]):
        raise ValueError('offsets must ascend')
    return array


def pooled_output(torch, offsets, out, dtype, col_off, dim, device, check_devices):
    """What Reader.bags_embedding_device and ReadersUnion.pooled_rows_device check alike once their rows are in order: the
    offsets, the dtype and the out of a pooled device lookup of rows on `device` into columns [col_off, col_off + dim).
    check_devices(out) raises the caller's own ValueError unless rows, offsets and out are where its kernel runs. Returns
    (bags, out, out_type, ld): out made where it was None, out_type the _memb.OUT_* of its dtype, ld its leading dimension
    in elements."""
    if (not isinstance(offsets, torch.Tensor) or offsets.device.type != 'cuda' or offsets.dtype not in (torch.int32, torch.uint32)
            or not offsets.is_contiguous() or offsets.dim() != 1):
        raise TypeError('offsets must be a contiguous int32/uint32 tensor of bags + 1 entries on the GPU')
    if offsets.numel() < 1:
        raise ValueError('offsets needs bags + 1 entries')
    bags = offsets.numel() - 1
    if dtype is None:
        if out is not None and out.dtype != torch.float32:
            raise TypeError('out is {}: pooled rows are float32 unless dtype asks for bfloat16 / float16'.format(out.dtype))
        dtype = torch.float32
    elif dtype not in (torch.float32, torch.bfloat16, torch.float16):
        raise TypeError('dtype must be torch.float32, torch.bfloat16 or torch.float16, not {}'.format(dtype))
    elif out is not None and out.dtype != dtype:
        raise TypeError('out is {} but dtype is {}'.format(out.dtype, dtype))
    if out is None:
        out = torch.empty((bags, col_off + dim), dtype=dtype, device=device)
    if out.dim() != 2 or out.stride(1) != 1 or out.shape[0] != bags:
        raise TypeError('out must be a {} (bags, width) tensor with unit column stride'.format(dtype))
    check_devices(out)
    if out.shape[1] < col_off + dim:
        raise ValueError('out is narrower than col_off + dim')
    out_type = {torch.float32: _memb.OUT_F32, torch.bfloat16: _memb.OUT_BF16, torch.float16: _memb.OUT_F16}[dtype]
    ld = out.stride(0) if bags > 1 else out.shape[1]
    return bags, out, out_type, ld


def flatten_sentences(sentences):
    """(words, offsets) of a sequence of word sequences: the sentences' words side by side and, as numpy.int64, where each
    sentence begins among them (len(sentences) + 1 entries)"""
    words = []
    offsets = np.zeros(len(sentences) + 1, dtype=np.int64)
    for position, sentence in enumerate(sentences):
        if isinstance(sentence, (str, bytes)):
            raise TypeError('a sentence is a sequence of words, not one string')
        words.extend(sentence)
        offsets[position + 1] = len(words)
    if len(words) > 0xFFFFFFFF:
        raise ValueError('more than 0xFFFFFFFF words in one call')
    return words, bag_offsets(offsets, len(words))   # (host-made: checked like a caller's)


def pool_slices_host(offsets, n, dim, slice_entries, mean, skip, slice_values):
    """The pooled lookup of include/memb_hip_pooled.h in numpy, for readers that decode on the host: the float32 sum or
    `mean` of each bag of n entries (offsets: bag_offsets), added in entry order, over slices of slice_entries entries so
    that no more than a slice of rows is ever decoded. slice_values(start, stop) is a generator that yields the float32
    (stop - start, dim) rows of the entries [start, stop). With `skip` (missing='skip': an unknown entry is left out of its
    bag and of the mean's count) it first yields the slice's boolean mask of known entries, then the rows of those entries
    alone; it is not asked for rows that no bag would use. Returns (out, known_counts): the (bags, dim) result and, with
    `skip`, the known entries of each bag as numpy.int64 (zeros without)."""
    bags = offsets.size - 1
    out = np.zeros((bags, dim), dtype=np.float32)
    begins, ends = offsets[:-1], offsets[1:]
    known_counts = np.zeros(bags, dtype=np.int64)   # skip: the bags' known entries in the slices so far
    for start in range(0, n, slice_entries):
        stop = min(n, start + slice_entries)
        first = int(np.searchsorted(ends, start, side='right'))    # the first bag that ends behind `start`
        last = int(np.searchsorted(begins, stop, side='left'))     # bags below this one begin before `stop`
        bag = np.arange(first, last)
        low = np.maximum(begins[first:last], start)
        high = np.minimum(ends[first:last], stop)
        fresh = begins[first:last] >= start                        # the bag's first entry lies in this slice
        keep = high > low
        bag, low, high, fresh = bag[keep], low[keep], high[keep], fresh[keep]
        if not bag.size:
            continue
        produced = slice_values(start, stop)
        if skip:
            # the slice's known entries side by side: a bag's range among them, and whether its sum starts here; only
            # they are decoded, and a slice without one is not decoded at all
            known = next(produced)
            if not known.any():
                continue
            before = np.concatenate(([0], np.cumsum(known)))
            low, high = before[low - start] + start, before[high - start] + start
            fresh = known_counts[bag] == 0
            known_counts[bag] += high - low
            keep = high > low
            bag, low, high, fresh = bag[keep], low[keep], high[keep], fresh[keep]
            if not bag.size:
                continue
        values = next(produced)
        for step in range(int((high - low).max())):
            active = (high - low) > step
            addend = values[low[active] + step - start]
            target = bag[active]
            if step == 0:
                begun = fresh[active]
                out[target[begun]] = addend[begun]
                out[target[~begun]] = out[target[~begun]] + addend[~begun]
            else:
                out[target] = out[target] + addend
    if mean:
        counts = (known_counts if skip else ends - begins).astype(np.float32)
        filled = counts > 0
        out[filled] = out[filled] / counts[filled][:, None]
    return out, known_counts


NORMS_HOST_CHUNK = 1 << 16      # rows row_norms / unit_rows_embedding of a device='cpu' reader decode at a time
NORMS_DEVICE_SLICE = 1 << 20    # rows row_norms_device decodes into a temporary at a time where no fused kernel exists
QUERY_DEVICE_SLICE = 1 << 19    # candidates query_similarity_device decodes beside their queries at a time where no fused kernel exists
UNIT_EPS = np.float32(1e-12)    # torch.nn.functional.normalize's eps


def _contract_sums(products):
    """The reduction include/memb_hip_norms.h and include/memb_hip_pairs.h share, over a float32 (n, 4 * pieces) matrix of
    products: piece sums ((t0 + t1) + t2) + t3, 64 lane partials over the pieces l, l + 64, .. (a lane without a further
    piece keeps its bits), a butterfly of strides 1 .. 32. Returns the float32 (n,) totals."""
    n = products.shape[0]
    pieces = products.shape[1] // 4
    terms = products.reshape(n, pieces, 4)
    sums = ((terms[:, :, 0] + terms[:, :, 1]) + terms[:, :, 2]) + terms[:, :, 3]
    partial = np.zeros((n, 64), dtype=np.float32)
    partial[:, :min(64, pieces)] = sums[:, :64]
    for first in range(64, pieces, 64):
        width = min(64, pieces - first)
        partial[:, :width] = partial[:, :width] + sums[:, first:first + width]
    lanes = np.arange(64)
    for stride in (1, 2, 4, 8, 16, 32):
        partial = partial + partial[:, lanes ^ stride]
    return partial[:, 0]


def _padded_to_pieces(values):
    """a float32 (n, dim) matrix with +0.0 columns up to a multiple of 4"""
    values = np.ascontiguousarray(values, dtype=np.float32)
    n, dim = values.shape
    padded = np.zeros((n, 4 * -(-dim // 4)), dtype=np.float32)
    padded[:, :dim] = values
    return padded


def row_norms_host(values):
    """The norm contract of include/memb_hip_norms.h in numpy: the float32 (n,) norms of the rows of a float32 (n, dim)
    matrix, every product, sum and root one IEEE float32 operation in the kernels' order -- piece sums
    ((v0 v0 + v1 v1) + v2 v2) + v3 v3 over columns 4k .. 4k + 3 (a column >= dim is +0.0), 64 lane partials over the pieces
    l, l + 64, .., a butterfly of strides 1 .. 32, one square root."""
    padded = _padded_to_pieces(values)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        return np.sqrt(_contract_sums(padded * padded))


def pair_similarity_host(x, y):
    """The contract of include/memb_hip_pairs.h in numpy for the pairs (x[i], y[i]) of two float32 (n, dim) matrices:
    (cosines, dots, norms), float32 (n,), (n,) and (n, 2). The dot is row_norms_host's reduction over the products x * y,
    the norms are row_norms_host's, cos = dot / (max(na, 1e-12) * max(nb, 1e-12)): one float32 product and one float32
    quotient, not clamped to [-1, 1]."""
    x, y = _padded_to_pieces(x), _padded_to_pieces(y)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        dots = _contract_sums(x * y)
        norms = np.stack([np.sqrt(_contract_sums(x * x)), np.sqrt(_contract_sums(y * y))], axis=1)
        floored = np.where(norms < UNIT_EPS, UNIT_EPS, norms)
        return dots / (floored[:, 0] * floored[:, 1]), dots, norms


def unit_rows_host(values, norms=None):
    """values / max(norm, 1e-12) row by row, one float32 division per element (include/memb_hip_norms.h); norms:
    row_norms_host(values) where the caller has them already."""
    values = np.ascontiguousarray(values, dtype=np.float32)
    if norms is None:
        norms = row_norms_host(values)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        return values / np.where(norms < UNIT_EPS, UNIT_EPS, norms)[:, None]


def weighted_rows_sum_host(values, weights, offsets):
    """The sums of include/memb_hip_analogies.h in numpy: for sum q over the entries offsets[q] .. offsets[q + 1] of the
    float32 (n, dim) matrix, in that order, from +0.0: out[q] = out[q] + (weights[e] * values[e]), the product and the sum
    each one float32 operation. weights: float32 (n,), None: all +1. Returns the float32 (Q, dim) sums."""
    values = np.ascontiguousarray(values, dtype=np.float32)
    offsets = np.asarray(offsets, dtype=np.int64)
    weights = np.ones(values.shape[0], dtype=np.float32) if weights is None else np.ascontiguousarray(weights, dtype=np.float32)
    begins, lengths = offsets[:-1], offsets[1:] - offsets[:-1]
    out = np.zeros((begins.size, values.shape[1]), dtype=np.float32)
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        for step in range(int(lengths.max()) if lengths.size else 0):
            sums = np.nonzero(lengths > step)[0]
            entries = begins[sums] + step
            out[sums] = out[sums] + weights[entries, None] * values[entries]
    return out


def cosmul_questions(offsets, negatives_from, n_terms):
    """The questions of include/memb_hip_cosmul.h checked on the host: (offsets int64 (Q + 1), negatives_from int64 (Q)).
    ValueError unless the offsets ascend within 0 .. n_terms, offsets[q] <= negatives_from[q] <= offsets[q + 1] and no
    question has more than COSMUL_MAX_TERMS terms."""
    offsets = np.asarray(offsets)
    negatives_from = np.asarray(negatives_from)
    if (offsets.size and offsets.dtype.kind not in 'iu') or (negatives_from.size and negatives_from.dtype.kind not in 'iu'):
        raise TypeError('offsets and negatives_from must be integer arrays')
    offsets = offsets.astype(np.int64).reshape(-1)
    negatives_from = negatives_from.astype(np.int64).reshape(-1)
    if offsets.size != negatives_from.size + 1:
        raise ValueError('offsets needs Q + 1 entries and negatives_from Q, got {} and {}'.format(offsets.size, negatives_from.size))
    if offsets[0] < 0 or offsets[-1] > n_terms or (offsets[1:] < offsets[:-1]).any():
        raise ValueError('offsets must ascend within 0 .. {} (the number of terms)'.format(n_terms))
    if (negatives_from < offsets[:-1]).any() or (negatives_from > offsets[1:]).any():
        raise ValueError('negatives_from[q] must lie within offsets[q] .. offsets[q + 1]')
    if negatives_from.size and int((offsets[1:] - offsets[:-1]).max()) > COSMUL_MAX_TERMS:
        raise ValueError('a question takes at most {} terms, got {}'.format(COSMUL_MAX_TERMS, int((offsets[1:] - offsets[:-1]).max())))
    return offsets, negatives_from


def cosmul_scores_host(cosines, offsets, negatives_from):
    """The 3CosMul scores of include/memb_hip_cosmul.h in numpy: for question q over the rows offsets[q] .. offsets[q + 1] of
    the float32 (T, n) matrix of cosines, the rows before negatives_from[q] positive and the others negative, each group in
    order: num = num * ((1 + c) * 0.5) from 1, den likewise, score = num / (den + 1e-6), every operation one float32
    operation. Returns the float32 (Q, n) scores."""
    cosines = np.ascontiguousarray(cosines, dtype=np.float32)
    offsets, negatives_from = cosmul_questions(offsets, negatives_from, cosines.shape[0])
    one, half, eps = np.float32(1), np.float32(0.5), np.float32(0.000001)
    num = np.ones((negatives_from.size, cosines.shape[1]), dtype=np.float32)
    den = np.ones_like(num)
    with np.errstate(over='ignore', under='ignore', invalid='ignore', divide='ignore'):
        for q in range(negatives_from.size):
            for term in range(int(offsets[q]), int(offsets[q + 1])):
                shifted = (one + cosines[term]) * half
                if term < negatives_from[q]:
                    num[q] = num[q] * shifted
                else:
                    den[q] = den[q] * shifted
        return num / (den + eps)


def rank_marks(thresholds, marks, count):
    """The marks of include/memb_hip_ranks.h checked on the host: (thresholds float32 (count,), marks int64 (count,));
    marks=None: all -1."""
    thresholds = np.asarray(thresholds)
    if thresholds.dtype != np.float32:
        raise TypeError('thresholds must be a float32 array of shape (Q,)')
    if thresholds.shape != (count,):
        raise ValueError('thresholds must have shape (Q,) = ({},), got {}'.format(count, thresholds.shape))
    if marks is None:
        marks = np.full(count, -1, dtype=np.int64)
    marks = np.asarray(marks)
    if marks.dtype.kind not in 'iu':
        raise TypeError('marks must be an integer array of shape (Q,)')
    if marks.shape != (count,):
        raise ValueError('marks must have shape (Q,) = ({},), got {}'.format(count, marks.shape))
    return np.ascontiguousarray(thresholds), np.ascontiguousarray(marks, dtype=np.int64)


def ranks_host(matrix, thresholds, marks, base=0, exclude=None):
    """The contract of include/memb_hip_ranks.h in numpy: the int64 (Q,) counts of the float32 (Q, n) matrix -- how many
    columns of row q precede the mark (thresholds[q], marks[q]), a column c being the position base + c: those whose key
    (topk_keys) is greater than the threshold's, and those with an equal key and a position below marks[q]. exclude:
    the list of non-candidates, an integer (Q, E) array of positions that are not counted; an entry outside
    [base, base + n) is ignored, repeats count once. Counts of slices of a matrix, each with its base, add up to the count
    of the whole."""
    return _precedes_host(matrix, thresholds, marks, base, exclude)[1].sum(axis=1, dtype=np.int64)


def _precedes_host(matrix, thresholds, marks, base, exclude):
    """(the matrix as contiguous float32, the bool (Q, n) array "column c of row q precedes the row's mark and is not named
    by the row's list"): the one predicate of ranks_host and within_host"""
    matrix = np.ascontiguousarray(matrix, dtype=np.float32)
    count, n = matrix.shape
    thresholds, marks = rank_marks(thresholds, marks, count)
    keys = topk_keys(matrix)
    mark_keys = topk_keys(thresholds)[:, None]
    positions = base + np.arange(n, dtype=np.int64)
    precedes = (keys > mark_keys) | ((keys == mark_keys) & (positions[None, :] < marks[:, None]))
    if exclude is not None:
        exclude = np.asarray(exclude, dtype=np.int64).reshape(count, -1)
        named = (exclude >= base) & (exclude < base + n)
        precedes[np.nonzero(named)[0], (exclude - np.where(named, base, exclude))[named]] = False
    return matrix, precedes


def within_host(matrix, thresholds, marks, base=0, exclude=None):
    """The contract of include/memb_hip_within.h in numpy: (offsets int64 (Q + 1,), positions int64 (total,), values
    float32 (total,)) of the float32 (Q, n) matrix -- the columns ranks_host counts, listed: row q's entries are
    positions[offsets[q]:offsets[q + 1]], base + column ascending, and values holds the matrix's bits there. The lists of
    slices of a matrix, each with its base, in ascending order of the bases, concatenate row by row to the lists of the
    whole."""
    matrix, precedes = _precedes_host(matrix, thresholds, marks, base, exclude)
    offsets = np.zeros(matrix.shape[0] + 1, dtype=np.int64)
    np.cumsum(precedes.sum(axis=1, dtype=np.int64), out=offsets[1:])
    found_rows, columns = np.nonzero(precedes)   # (row by row, the columns of a row ascending)
    return offsets, base + columns.astype(np.int64), matrix[found_rows, columns]


QUERY_BAGS_DEVICE_SLICE = 1 << 16   # bags bag_similarity_matrix_device pools into a temporary at a time where no fused kernel exists
QUERY_BAGS_HOST_SLICE = 1 << 12     # bags bag_similarity_matrix of a device='cpu' reader pools at a time
COSMUL_MAX_TERMS = _memb_cosmul.COSMUL_MAX_TERMS   # terms per 3CosMul question (MEMB_HIP_COSMUL_MAX_TERMS)
QUERY_TOPK_MAX_K = _memb.QUERY_TOPK_MAX_K   # one rank per lane of a wavefront (MEMB_HIP_TOPK_MAX_K)
QUERY_TOPK_MAX_EXCLUDED = _memb.QUERY_TOPK_MAX_EXCLUDED   # excluded positions per query, one per lane (MEMB_HIP_MAX_EXCLUDED)


def topk_size(k, spare=0):
    """k as an int; ValueError unless 1 <= k <= QUERY_TOPK_MAX_K - spare"""
    if isinstance(k, bool) or int(k) != k:
        raise TypeError('k must be an integer')
    if not 1 <= k <= QUERY_TOPK_MAX_K - spare:
        raise ValueError('k must be 1 .. {} (the selection keeps at most {} entries per query{}), got {}'.format(
            QUERY_TOPK_MAX_K - spare, QUERY_TOPK_MAX_K, ', one of them the word itself' if spare else '', k))
    return int(k)


def topk_fallback_list_bytes(count, n, k, slice_size):
    """The bytes of segment lists similarity_topk_device's fallback needs for its dense_topk_to_device calls over n
    candidates in slices of slice_size: the larger of what a full slice and what the shorter last slice ask for. A shorter
    slice can need MORE: segments are whole multiples of 256 columns, so fewer columns may be cut into more segments (33
    queries: 228 segments for 524 288 columns, 249 for 509 952)."""
    sizes = {min(n, slice_size)}
    if n > slice_size and n % slice_size:
        sizes.add(n % slice_size)
    return max(_memb.dense_topk_workspace_bytes(count, size, k) for size in sizes)


def topk_keys(values):
    """include/memb_hip_query_topk.h's order on float32 values as uint32 keys, greater first: every NaN the one greatest
    key, -0.0 the key of +0.0, -inf the smallest; no value has key 0"""
    bits = np.ascontiguousarray(values, dtype=np.float32).view(np.uint32)
    bits = np.where(bits == np.uint32(0x80000000), np.uint32(0), bits)
    keys = np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000))
    return np.where((bits & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000), np.uint32(0xFFFFFFFF), keys).astype(np.uint32)


def topk_host(matrix, k, base=0, held=None, exclude=None):
    """The contract of include/memb_hip_query_topk.h in numpy: (values float32 (Q, k), positions int64 (Q, k)) of the
    float32 (Q, n) matrix, positions as base + column; held: a (values, positions) pair of an earlier call whose entries
    (position -1: empty) take part, their positions outside [base, base + n). exclude: include/memb_hip_analogies.h's
    list, an integer (Q, E) array of positions that are no candidates of their row; an entry outside [base, base + n) is
    ignored."""
    matrix = np.ascontiguousarray(matrix, dtype=np.float32)
    count, n = matrix.shape
    bits = matrix.view(np.uint32)
    positions = np.broadcast_to(base + np.arange(n, dtype=np.int64), (count, n))
    keys = topk_keys(matrix).astype(np.int64)
    if exclude is not None:
        columns = np.asarray(exclude, dtype=np.int64).reshape(count, -1) - base
        named = (columns >= 0) & (columns < n)
        keys[np.nonzero(named)[0], columns[named]] = 0   # (an empty entry: behind every real one, stored as empty)
    if held is not None:
        bits = np.concatenate([held[0].view(np.uint32), bits], axis=1)
        keys = np.concatenate([np.where(held[1] < 0, 0, topk_keys(held[0]).astype(np.int64)), keys], axis=1)
        positions = np.concatenate([held[1], positions], axis=1)
    # key descending, then position ascending; an empty entry (key 0) behind every real one
    order = np.lexsort((positions, -keys), axis=1)[:, :k]
    keys = np.take_along_axis(keys, order, axis=1)
    values = np.full((count, k), 0xFF800000, dtype=np.uint32)
    found = np.full((count, k), -1, dtype=np.int64)
    width = order.shape[1]
    values[:, :width] = np.where(keys > 0, np.take_along_axis(bits, order, axis=1), np.uint32(0xFF800000))
    found[:, :width] = np.where(keys > 0, np.take_along_axis(positions, order, axis=1), -1)
    return values.view(np.float32), found


def tokenizer_word_list(tokenizer):
    """The words of a keras Tokenizer placed at their indices, '' where an index
    has no word (index 0 never has one). With `num_words` set only indices below
    it are kept, as the reference does (python/memb/reader.py:100-109); the
    embedding matrix of the tokenizer is then batch_embedding of this list."""
    entries = list(tokenizer.word_index.items())
    limit = tokenizer.num_words
    if limit is None:
        limit = max(index for _, index in entries) + 1
    else:
        entries = [(word, index) for word, index in entries if index < limit]
    slots = [''] * limit
    for word, index in entries:
        slots[index] = word
    return slots


class Reader(BaseReader):
    """One memb file, staged to a GPU on first use; lookups decode there.

    filename     str or path-like
    num_threads  host threads for the word search of large batches, 0 = one per core
    device       HIP device index (not in the reference API); default: environment
                 variable MEMB_HIP_DEVICE, else 0. 'cpu': decode on the host -- the reference's
                 own serial / threaded CPU path restated, for hosts without a GPU; it is only
                 ever used when asked for (a reader on a HIP device never falls back to it)
    host_below   host batches (words in, numpy out) of at most this many words are decoded on
                 the host although the reader lives on a GPU: a single word then costs no kernel
                 launch and no PCIe round trip. 0 = never (default, or MEMB_HOST_BELOW)
    max_direct_decode_bits
                 width of the first-level decode table, 0 = library default (results
                 never depend on it; the reference's tests force 1, src/tests.cpp:76-88)

    Footprint: the model itself (info()['device_bytes']) is staged on first use. Batches of 4096 words
    and more -- host results too -- are also SEARCHED on the device: the first such call copies the keys
    to HBM and builds a hash table over them there (16-byte slots, at least 2 x len(reader) of them, plus
    the keys: about 160 MB and some tens of milliseconds for a 2.2 M-word model; info()['word_index_bytes']).
    stage_words() pays that up front; device='cpu' and host_below keep a reader's host batches off it.
    """

    def __init__(self, filename, num_threads=0, device=None, max_direct_decode_bits=0, host_below=None):
        super().__init__()
        name = str(filename)
        if device in ('cpu', 'host'):
            device = _memb.HOST_DEVICE
        if device is None and not max_direct_decode_bits:
            self._impl = _memb.Reader(name, num_threads)
        else:
            self._impl = _memb.Reader(name, num_threads, -1 if device is None else int(device), max_direct_decode_bits)
        if host_below is not None:
            self._impl.set_host_below(int(host_below))
        self._word_batches = WordBatches()   # of resolve_rows_device / resolve_packed_device: one per call in flight
        self._last_norms_kernel = ''
        self._last_pairs_kernel = ''
        self._last_bag_pairs_kernel = ''
        self._last_query_kernel = ''
        self._last_query_matrix_kernel = ''
        self._last_query_topk_kernel = ''
        self._last_cosmul_kernel = ''
        self._last_ranks_kernel = ''
        self._last_within_kernel = ''
        self._last_query_bags_kernel = ''
        self._last_query_bags_topk_kernel = ''
        self._all_rows = None              # every row id in order on the device, of similarity_topk_device(rows=None)
        self._all_rows_lock = threading.Lock()
        self._whole_group_offsets = None   # ((n, device), the device tensor [0, n]) of query_similarity_device(offsets=None)

    @property
    def _word_batch(self):
        """the word batch a call of this reader gave back most recently (tests and measurement hooks look up its packed
        words again); None before the first call"""
        return self._word_batches.last

    @property
    def dim(self):
        """length of every vector"""
        return self._impl.dim()

    @property
    def device(self):
        """HIP device index, or 'cpu' for a reader that decodes on the host"""
        index = self._impl.device()
        return 'cpu' if index == _memb.HOST_DEVICE else index

    @property
    def host_rows_decoded(self):
        """rows decoded by the host path so far (0 for a GPU reader with default settings)"""
        return self._impl.host_rows_decoded()

    def __len__(self):
        return self._impl.size()

    def keys(self):
        """all words of the model, sorted"""
        return self._impl.keys()

    def word_embedding(self, word):
        """float32 vector of shape (dim,); zeros for an unknown word"""
        return self._impl.word_embedding(word)

    def batch_embedding(self, words):
        """float32 matrix of shape (len(words), dim), one row per word in the given
        order; rows of unknown words are zeros"""
        return self._impl.batch_embedding(words)

    def tokenizer_embedding(self, tokenizer):
        """weights for an Embedding layer indexed like the keras Tokenizer"""
        return self.batch_embedding(tokenizer_word_list(tokenizer))

    def to_keyed_vectors(self):
        """The whole model as a gensim KeyedVectors. The reference looks every key up again (python/memb/reader.py:27-28:
        batch_embedding(keys())); keys() IS the row order, so the rows are decoded by number and nothing is searched
        (SURVEY 8f-1's fast path) -- the same matrix."""
        try:
            from gensim.models import KeyedVectors
        except ImportError:
            raise ImportError('You must install gensim for KeyedVectors export')
        vocabulary = self.keys()
        exported = KeyedVectors(self.dim)
        exported.add(vocabulary, self.rows_embedding(np.arange(len(vocabulary), dtype=np.uint32)))
        return exported

    # ---- additions: row ids and device-resident results ----

    def resolve_rows(self, words):
        '''Row ids (positions in sorted key order) as numpy.uint32;
        0xFFFFFFFF marks words that are not in the model'''
        return self._impl.resolve_rows(words)

    def rows_embedding(self, rows):
        '''batch_embedding for already resolved row ids'''
        return self._impl.rows_embedding(np.ascontiguousarray(rows, dtype=np.uint32))

    def rows_embedding_into(self, rows, out, col_off=0):
        '''rows_embedding into columns [col_off, col_off + dim) of a C-contiguous float32 matrix
        (or a row range of one: slices of a shared result can be filled from several threads)'''
        self._impl.rows_embedding_into(np.ascontiguousarray(rows, dtype=np.uint32), out, col_off)

    def batch_embedding_into(self, words, out, col_off=0):
        '''Write the batch into columns [col_off, col_off + dim) of a wider float32 matrix'''
        self._impl.batch_embedding_into(words, out, col_off)

    def rows_embedding_device(self, rows, out=None, col_off=0, accumulate=False, divisor=0.0, order=None, dtype=None):
        '''Lookup that never leaves the GPU.
        Parameters
        ----------
        rows : torch.Tensor (int32 view of the uint32 row ids, on this reader's device)
        out : torch.Tensor of `dtype`, (n, >= col_off + dim) on the same device, optional
        accumulate : add the rows to what `out` holds instead of overwriting it (float32 only)
        divisor : if non-zero, divide the (accumulated) rows by it (float32 only)
        order : None, or 'random' -- a hint that the rows come in no particular order (token ids, shuffled keys): batches
            of more than 524 000 rows then keep blocks of four wavefronts, 3 % faster for such rows (key-order dumps like
            the default of eight). Never changes a result.
        dtype : torch.float32, torch.bfloat16 or torch.float16; default out.dtype, else float32. bf16 / fp16 rows are the
            float32 rows rounded once to nearest even (the bits of .to(dtype)), decoded straight into that type: no float32
            temporary, no second kernel.
        '''
        # (a small batch is seven microseconds of which the kernel is three: every attribute is fetched once)
        import torch
        device = rows.device
        if device.type != 'cuda' or rows.dtype not in (torch.int32, torch.uint32) or not rows.is_contiguous():
            raise TypeError('rows must be a contiguous int32/uint32 tensor on the GPU')
        if dtype is None:
            dtype = torch.float32 if out is None else out.dtype
        elif out is not None and out.dtype != dtype:
            raise TypeError('out is {} but dtype is {}'.format(out.dtype, dtype))
        if dtype not in (torch.float32, torch.bfloat16, torch.float16):
            raise TypeError('out must be a float32, bfloat16 or float16 (n, width) tensor with unit column stride')
        narrow = dtype != torch.float32
        if narrow and (accumulate or divisor):
            raise ValueError('accumulate and divisor need float32 rows: a {} sum would be rounded after every reader'.format(dtype))
        n = rows.numel()
        if out is None:
            out = torch.empty((n, col_off + self.dim), dtype=dtype, device=device)
        if out.dim() != 2 or out.stride(1) != 1 or out.shape[0] != n:
            raise TypeError('out must be a {} (n, width) tensor with unit column stride'.format(dtype))
        # the kernel runs on this reader's device with these pointers: both tensors must live there
        index = device.index
        if index != self._impl.device() or out.device != device:
            raise ValueError('rows and out must be on cuda:{} (the device this reader is staged on), got {} and {}'.format(
                self.device, device, out.device))
        if narrow:
            self._impl.rows_to_device_typed(
                rows.data_ptr(), n, out.data_ptr(), _memb.OUT_BF16 if dtype == torch.bfloat16 else _memb.OUT_F16,
                out.stride(0), col_off, _current_stream(torch, index))
            return out
        self._impl.rows_to_device(
            rows.data_ptr(), n, out.data_ptr(), out.stride(0), col_off, _current_stream(torch, index), accumulate, float(divisor),
            order == 'random')
        return out

    def bags_embedding_device(self, rows, offsets, mode='mean', out=None, col_off=0, dtype=None, missing='zero',
                              return_counts=False, reduction='sequential'):
        '''Pooled lookup that never leaves the GPU: the sum or mean of each bag of rows, decoded and reduced by one kernel
        (the EmbeddingBag counterpart of rows_embedding_device). The bags' rows are never written: per entry the kernel
        reads the row id and the compressed row, per bag it stores dim elements.
        Parameters
        ----------
        rows : torch.Tensor, as in rows_embedding_device (n entries)
        offsets : contiguous int32 / uint32 torch.Tensor of bags + 1 entries on this reader's device; bag b owns the
            entries [min(offsets[b], n), min(offsets[b + 1], n)) and is empty when that range is (offsets are read as
            uint32; no entry outside rows is read whatever they hold)
        mode : 'mean' or 'sum'. Both add a bag's float32 rows one after the other in entry order (a row that is not in
            the model is +0.0 and counts); 'mean' then divides once by the entry count. An empty bag is +0.0, a bag of
            one entry that row's bits. Bit for bit the result of that loop over rows_embedding_device(rows).
        out : torch.Tensor (bags, >= col_off + dim) with unit column stride on the same device, optional: float32, or of
            `dtype` where one is given
        dtype : None (float32), torch.float32, torch.bfloat16 or torch.float16. A bf16 / fp16 result is the float32 result
            rounded once to nearest even (the bits of .to(dtype)): the sums and the division stay float32 and only the
            finished value is narrowed as the same kernel stores it -- no float32 (bags, dim) temporary, no second kernel. A
            narrow result is asked for by name: a bf16 / fp16 `out` without `dtype` is a TypeError.
        missing : 'zero' (the default: the loop above) or 'skip'. With 'skip' an entry that is not in the model -- 0xFFFFFFFF
            or any id >= len(reader) -- is left out of its bag, as torch.nn.EmbeddingBag leaves out padding_idx: it adds
            nothing, not even +0.0 (a bag [missing, row of -0.0] is -0.0), and 'mean' divides by the number of KNOWN
            entries. A bag without a known entry is +0.0. Still one kernel: no compaction of ids or offsets. Bit for bit
            the missing='zero' result for the batch with the unknown entries taken out.
        return_counts : True returns (vectors, counts), counts a torch.int32 tensor of shape (bags,) on the device: the
            known entries of each bag. With missing='skip' only; a ValueError otherwise.
        reduction : 'sequential' (the default: the loops above, one wavefront per bag) or 'chunked', for LONG bags --
            documents, paragraphs. A bag is cut into chunks of memb_amd.POOL_CHUNK entries, chunk j owning the entries
            [begin + C j, min(end, begin + C (j + 1))); many wavefronts sum the chunks at once with the loop above, and the
            chunks' float32 sums are then added in chunk order, one IEEE addition each (with missing='skip' a chunk
            without a known entry adds nothing); 'mean' divides once by the bag's count. The order is fixed by the
            inputs alone; a bag of at most POOL_CHUNK entries has the bits of 'sequential'. Bit for bit mode='sum' of
            the sequential path over the chunks as bags, then that loop. Every bag's sum crosses a float32 workspace
            once (a torch tensor of this call): for short bags 'sequential' stays the faster choice. offsets must
            ascend; where they do not, the bags at and behind a decrease hold unspecified values.
        No accumulate into `out`, no per-entry weights, no 'max'.
        '''
        import torch
        code = pool_mode(mode)
        skip = pool_missing(missing, return_counts)
        chunked = pool_reduction(reduction)
        index = self._impl.device()
        if index == _memb.HOST_DEVICE:
            raise RuntimeError("this reader decodes on the host (device 'cpu'): device buffers need a reader on a HIP device")
        device = rows.device
        if device.type != 'cuda' or rows.dtype not in (torch.int32, torch.uint32) or not rows.is_contiguous():
            raise TypeError('rows must be a contiguous int32/uint32 tensor on the GPU')

        def check_devices(out):
            if device.index != index or out.device != device or offsets.device != device:
                raise ValueError('rows, offsets and out must be on cuda:{} (the device this reader is staged on), got {}, {} and {}'.format(
                    self.device, device, offsets.device, out.device))

        bags, out, out_type, ld = pooled_output(torch, offsets, out, dtype, col_off, self.dim, device, check_devices)
        if chunked:
            counts = torch.empty((bags,), dtype=torch.int32, device=device) if return_counts else None
            workspace_bytes = self._impl.pool_chunked_workspace_bytes(rows.numel(), bags)
            # this call's own: torch's allocator keeps it alive for the work enqueued on the current stream
            workspace = torch.empty((workspace_bytes,), dtype=torch.uint8, device=device)
            self._impl.pool_rows_chunked_to_device(
                rows.data_ptr(), rows.numel(), offsets.data_ptr(), bags, out.data_ptr(), ld, col_off, code,
                _current_stream(torch, index), out_type, skip, counts.data_ptr() if return_counts else 0,
                workspace.data_ptr(), workspace_bytes)
            return (out, counts) if return_counts else out
        if skip:
            counts = torch.empty((bags,), dtype=torch.int32, device=device) if return_counts else None
            self._impl.pool_known_rows_to_device(
                rows.data_ptr(), rows.numel(), offsets.data_ptr(), bags, out.data_ptr(), ld, col_off, code,
                _current_stream(torch, index), out_type, counts.data_ptr() if return_counts else 0)
            return (out, counts) if return_counts else out
        self._impl.pool_rows_to_device(
            rows.data_ptr(), rows.numel(), offsets.data_ptr(), bags, out.data_ptr(), ld, col_off, code,
            _current_stream(torch, index), out_type)
        return out

    def sentences_embedding_device(self, sentences, mode='mean', dtype=None, missing='zero', return_counts=False,
                                   reduction='sequential'):
        '''One vector per sentence, left on the GPU: `sentences` is a sequence of word sequences; the words are resolved on
        the device (resolve_rows_device) and each sentence's rows are pooled by bags_embedding_device -- words never
        become rows on the host. A sentence without words is a zero vector. Returns a (len(sentences), dim) tensor of
        `dtype` (bags_embedding_device: float32 by default; torch.bfloat16 / torch.float16 are that result rounded once).
        missing='skip' leaves the words the model does not know out of their sentences -- the mean is over the known words,
        a sentence of unknown words is a zero vector -- and return_counts=True then returns (vectors, counts), the known
        words per sentence (bags_embedding_device). reduction='chunked' pools long sentences -- documents -- under
        bags_embedding_device's chunked order.'''
        import torch
        pool_mode(mode)
        pool_missing(missing, return_counts)
        pool_reduction(reduction)
        index = self._impl.device()
        if index == _memb.HOST_DEVICE:
            raise RuntimeError("this reader decodes on the host (device 'cpu'): device buffers need a reader on a HIP device")
        words, offsets = flatten_sentences(sentences)
        device = 'cuda:{}'.format(index)
        rows = self.resolve_rows_device(words) if words else torch.empty((0,), dtype=torch.int32, device=device)
        on_device = torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).to(device)
        return self.bags_embedding_device(
            rows, on_device, mode=mode, dtype=dtype, missing=missing, return_counts=return_counts, reduction=reduction)

    def bags_embedding(self, rows, offsets, mode='mean', missing='zero', return_counts=False, reduction='sequential'):
        '''bags_embedding_device for host arrays: numpy row ids and offsets in, a numpy float32 (bags, dim) matrix out.
        offsets: bags + 1 integers, ascending, within 0 .. len(rows) -- anything else is a ValueError. A reader on a GPU
        sends the ids and offsets up and brings only bags x dim floats back (PCIe bounds the host API). A device='cpu'
        reader decodes rows_embedding in bounded chunks and adds them in entry order in numpy: the same bits.
        missing='skip' leaves the entries that are not in the model out of their bags (bags_embedding_device), on either
        path; return_counts=True then returns (vectors, counts), counts a numpy.uint32 array of the bags' known entries.
        reduction='chunked' is bags_embedding_device's chunked order, on either path with the same bits.'''
        code = pool_mode(mode)
        skip = pool_missing(missing, return_counts)
        chunked = pool_reduction(reduction)
        rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
        offsets = bag_offsets(offsets, rows.size)
        if self._impl.device() != _memb.HOST_DEVICE:
            import torch
            device = 'cuda:{}'.format(self._impl.device())
            result = self.bags_embedding_device(
                torch.from_numpy(rows.view(np.int32)).to(device),
                torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).to(device), mode=mode, missing=missing,
                return_counts=return_counts, reduction=reduction)
            if return_counts:
                return result[0].cpu().numpy(), result[1].cpu().numpy().view(np.uint32)
            return result.cpu().numpy()
        if chunked:
            return self._bags_embedding_chunked(rows, offsets, code, skip, return_counts)

        def slice_values(start, stop):
            if skip:
                known = rows[start:stop] < len(self)
                yield known
                yield self.rows_embedding(rows[start:stop][known])
            else:
                yield self.rows_embedding(rows[start:stop])

        out, known_counts = pool_slices_host(
            offsets, rows.size, self.dim, BAGS_HOST_CHUNK, code == _memb.POOL_MEAN, skip, slice_values)
        if return_counts:
            return out, known_counts.astype(np.uint32)
        return out

    def _bags_embedding_chunked(self, rows, offsets, code, skip, return_counts):
        """bags_embedding(reduction='chunked') of a device='cpu' reader: the sequential sums of the chunks as bags, then the
        chunks' sums added in chunk order, all bags at once per step."""
        bags = offsets.size - 1
        derived, first = chunk_offsets(offsets)
        if skip:
            partial, chunk_counts = self.bags_embedding(rows, derived, mode='sum', missing='skip', return_counts=True)
            chunk_counts = chunk_counts.astype(np.int64)
        else:
            partial = self.bags_embedding(rows, derived, mode='sum')
            chunk_counts = np.ones(derived.size - 1, dtype=np.int64)   # every chunk counts, an empty bag's one too
        out = np.zeros((bags, self.dim), dtype=np.float32)
        started = np.zeros(bags, dtype=bool)
        per_bag = first[1:] - first[:-1]
        for step in range(int(per_bag.max()) if bags else 0):
            bag = np.nonzero(per_bag > step)[0]
            chunk = first[bag] + step
            used = chunk_counts[chunk] > 0
            bag, chunk = bag[used], chunk[used]
            fresh = ~started[bag]
            out[bag[fresh]] = partial[chunk[fresh]]
            out[bag[~fresh]] = out[bag[~fresh]] + partial[chunk[~fresh]]
            started[bag] = True
        known_counts = np.add.reduceat(chunk_counts, first[:-1]) if bags else np.zeros(0, dtype=np.int64)
        if code == _memb.POOL_MEAN:
            counts = (known_counts if skip else offsets[1:] - offsets[:-1]).astype(np.float32)
            filled = counts > 0
            out[filled] = out[filled] / counts[filled][:, None]
        if return_counts:
            return out, known_counts.astype(np.uint32)
        return out

    @property
    def last_norms_kernel(self):
        """The kernel family of the last row_norms_device / unit_rows_embedding_device call: 'norms_trained' /
        'unit_trained' (fused with the decode), or 'norms_dense' / 'unit_dense' behind a plain decode of the rows -- uniform
        and full storage, dims that are no multiple of 4 or beyond 512, unit rows whose output is not aligned to 16 bytes.
        '' before any call. Informational: the bits are the same."""
        return self._last_norms_kernel

    def _norms_arguments(self, torch, rows):
        """the checks row_norms_device and unit_rows_embedding_device share with rows_embedding_device"""
        index = self._impl.device()
        if index == _memb.HOST_DEVICE:
            raise RuntimeError("this reader decodes on the host (device 'cpu'): device buffers need a reader on a HIP device")
        device = rows.device
        if device.type != 'cuda' or rows.dtype not in (torch.int32, torch.uint32) or not rows.is_contiguous():
            raise TypeError('rows must be a contiguous int32/uint32 tensor on the GPU')
        return index, device

    def row_norms_device(self, rows, out=None):
        '''The Euclidean norm of each row, left on the GPU: a float32 (n,) tensor. For trained models whose dim is a
        multiple of 4 and at most 512 ONE kernel computes it from the compressed rows and writes no row; otherwise the
        rows are decoded in slices of at most 2^20 into a temporary and reduced there (last_norms_kernel says which). Bit
        for bit the contract of include/memb_hip_norms.h over rows_embedding_device(rows): float32 piece sums, a fixed
        reduction tree, a correctly rounded root -- whichever kernel ran. A row that is not in the model has norm 0.
        rows : torch.Tensor, as in rows_embedding_device
        out : optional contiguous float32 (n,) tensor on the same device'''
        import torch
        index, device = self._norms_arguments(torch, rows)
        n = rows.numel()
        if out is None:
            out = torch.empty((n,), dtype=torch.float32, device=device)
        if out.dtype != torch.float32 or out.dim() != 1 or out.shape[0] != n or not out.is_contiguous():
            raise TypeError('out must be a contiguous float32 (n,) tensor')
        if device.index != index or out.device != device:
            raise ValueError('rows and out must be on cuda:{} (the device this reader is staged on), got {} and {}'.format(
                self.device, device, out.device))
        stream = _current_stream(torch, index)
        if self._impl.row_norms_to_device(rows.data_ptr(), n, out.data_ptr(), stream):
            self._last_norms_kernel = self._impl.norms_kernel_name(False)
            return out
        flat = rows.reshape(-1)
        dim = self.dim
        temporary = torch.empty((min(n, NORMS_DEVICE_SLICE), dim), dtype=torch.float32, device=device)
        for start in range(0, n, NORMS_DEVICE_SLICE):
            stop = min(n, start + NORMS_DEVICE_SLICE)
            decoded = self.rows_embedding_device(flat[start:stop], out=temporary[:stop - start])
            _memb.dense_row_norms_to_device(index, decoded.data_ptr(), stop - start, dim, dim, out[start:stop].data_ptr(), stream)
        self._last_norms_kernel = _memb.dense_norms_kernel_name(False)
        return out

    def unit_rows_embedding_device(self, rows, out=None, col_off=0, return_norms=False):
        '''rows_embedding_device with every row divided by max(its norm, 1e-12) -- torch.nn.functional.normalize's
        definition -- in the kernel that decodes it where row_norms_device's fused form exists and every row of `out` is
        aligned to 16 bytes; otherwise the plain decode into `out` and a second kernel in place (last_norms_kernel says
        which): no temporary either way. Bit for bit the contract of include/memb_hip_norms.h: row_norms_device's norm, one
        correctly rounded float32 division per element. A missing or all-zero row stays zeros.
        out : float32 (n, >= col_off + dim) tensor with unit column stride on the same device, optional; nothing outside
            columns [col_off, col_off + dim) is written
        return_norms : True returns (rows, norms), norms the float32 (n,) tensor of row_norms_device
        float32 only: no bfloat16 / float16 unit rows.'''
        import torch
        index, device = self._norms_arguments(torch, rows)
        n = rows.numel()
        dim = self.dim
        if out is None:
            out = torch.empty((n, col_off + dim), dtype=torch.float32, device=device)
        if out.dtype != torch.float32 or out.dim() != 2 or out.stride(1) != 1 or out.shape[0] != n:
            raise TypeError('out must be a float32 (n, width) tensor with unit column stride')
        if device.index != index or out.device != device:
            raise ValueError('rows and out must be on cuda:{} (the device this reader is staged on), got {} and {}'.format(
                self.device, device, out.device))
        if out.shape[1] < col_off + dim:
            raise ValueError('out is narrower than col_off + dim')
        norms = torch.empty((n,), dtype=torch.float32, device=device) if return_norms else None
        ld = out.stride(0) if n > 1 else out.shape[1]
        self._impl.unit_rows_to_device(
            rows.data_ptr(), n, out.data_ptr(), ld, col_off, norms.data_ptr() if return_norms else 0,
            _current_stream(torch, index))
        self._last_norms_kernel = self._impl.norms_kernel_name(True, out.data_ptr(), ld, col_off)
        return (out, norms) if return_norms else out

    def unit_batch_embedding_device(self, words):
        '''batch_embedding_device with rows of unit length (unit_rows_embedding_device); an unknown word stays zeros'''
        return self.unit_rows_embedding_device(self.resolve_rows_device(words))

    def row_norms(self, rows):
        '''row_norms_device for host arrays: numpy row ids in, a numpy float32 (n,) array out. A reader on a GPU sends the
        ids up and brings n floats back; a device='cpu' reader evaluates the same contract in numpy over rows_embedding in
        bounded slices: the same bits.'''
        rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
        if self._impl.device() != _memb.HOST_DEVICE:
            import torch
            on_device = torch.from_numpy(rows.view(np.int32)).to('cuda:{}'.format(self._impl.device()))
            return self.row_norms_device(on_device).cpu().numpy()
        out = np.zeros(rows.size, dtype=np.float32)
        for start in range(0, rows.size, NORMS_HOST_CHUNK):
            out[start:start + NORMS_HOST_CHUNK] = row_norms_host(self.rows_embedding(rows[start:start + NORMS_HOST_CHUNK]))
        return out

    def unit_rows_embedding(self, rows):
        '''unit_rows_embedding_device for host arrays: a numpy float32 (n, dim) matrix of unit rows, on either path with
        the same bits (row_norms)'''
        rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
        if self._impl.device() != _memb.HOST_DEVICE:
            import torch
            on_device = torch.from_numpy(rows.view(np.int32)).to('cuda:{}'.format(self._impl.device()))
            return self.unit_rows_embedding_device(on_device).cpu().numpy()
        out = np.zeros((rows.size, self.dim), dtype=np.float32)
        for start in range(0, rows.size, NORMS_HOST_CHUNK):
            out[start:start + NORMS_HOST_CHUNK] = unit_rows_host(self.rows_embedding(rows[start:start + NORMS_HOST_CHUNK]))
        return out

    @property
    def last_pairs_kernel(self):
        """The kernel family of the last pair_similarity_device call: 'pairs_trained' (fused with the decode) or
        'pairs_dense' behind a plain decode of the rows -- uniform and full storage, dims that are no multiple of 4 or
        beyond 512, geometries of one word per wavefront. '' before any call. Informational: the bits are the same."""
        return self._last_pairs_kernel

    def pair_similarity_device(self, rows_a, rows_b=None, *, return_dots=False, return_norms=False, out=None):
        '''The cosine similarity of pairs of rows, left on the GPU: a float32 (n,) tensor, cos[i] of the rows rows_a[i] and
        rows_b[i]. For trained models whose dim is a multiple of 4 and at most 512 ONE kernel computes it from the
        compressed rows and writes no row; otherwise the rows are decoded in slices of at most 2^20 into a temporary and
        reduced there (last_pairs_kernel says which). Bit for bit the contract of include/memb_hip_pairs.h over
        rows_embedding_device: float32 piece products, row_norms_device's reduction tree and norms,
        cos = dot / (max(na, 1e-12) * max(nb, 1e-12)) -- whichever kernel ran. Not clamped: the cosine of a row with itself
        may be 1.0000001. A pair with a row that is not in the model has cosine 0.
        rows_a, rows_b : two contiguous int32 / uint32 (n,) tensors on this reader's device, as in rows_embedding_device
            (they are interleaved by one torch.stack), or rows_b=None and rows_a a contiguous (n, 2) tensor of pairs, which
            is passed as it is: nothing is allocated but the results
        return_dots, return_norms : either one returns (cosines, dots, norms) instead, dots a float32 (n,) and norms a
            float32 (n, 2) tensor -- row_norms_device's of rows_a and rows_b --, None where not asked for
        out : optional contiguous float32 (n,) tensor on the same device for the cosines
        One model, float32 only: no ReadersUnion, no ShardedReader, no bfloat16 / float16, no one-against-many search.'''
        import torch
        index, device = self._norms_arguments(torch, rows_a)
        if rows_b is None:
            if rows_a.dim() != 2 or rows_a.shape[1] != 2:
                raise TypeError('without rows_b, rows_a must be a contiguous (n, 2) tensor of pairs')
            pairs = rows_a
        else:
            self._norms_arguments(torch, rows_b)
            if rows_a.dim() != 1 or rows_b.shape != rows_a.shape or rows_b.dtype != rows_a.dtype or rows_b.device != device:
                raise TypeError('rows_a and rows_b must be (n,) tensors of one dtype on one device')
            pairs = torch.stack((rows_a.view(torch.int32), rows_b.view(torch.int32)), dim=1)   # (the ids' bits)
        n = pairs.shape[0]
        if out is None:
            out = torch.empty((n,), dtype=torch.float32, device=device)
        if out.dtype != torch.float32 or out.dim() != 1 or out.shape[0] != n or not out.is_contiguous():
            raise TypeError('out must be a contiguous float32 (n,) tensor')
        if device.index != index or out.device != device:
            raise ValueError('rows and out must be on cuda:{} (the device this reader is staged on), got {} and {}'.format(
                self.device, device, out.device))
        dots = torch.empty((n,), dtype=torch.float32, device=device) if return_dots else None
        norms = torch.empty((n, 2), dtype=torch.float32, device=device) if return_norms else None
        result = (out, dots, norms) if return_dots or return_norms else out

        def pointers(start, stop):
            return (out[start:stop].data_ptr(), dots[start:stop].data_ptr() if return_dots else 0,
                    norms[start:stop].data_ptr() if return_norms else 0)

        stream = _current_stream(torch, index)
        if self._impl.pair_similarity_to_device(pairs.data_ptr(), n, *pointers(0, n), stream):
            self._last_pairs_kernel = self._impl.pairs_kernel_name()
            return result
        flat = pairs.reshape(-1)
        dim = self.dim
        slice_pairs = max(NORMS_DEVICE_SLICE // 2, 1)   # slices of at most NORMS_DEVICE_SLICE rows, an even number
        temporary = torch.empty((2 * min(n, slice_pairs), dim), dtype=torch.float32, device=device)
        for start in range(0, n, slice_pairs):
            stop = min(n, start + slice_pairs)
            decoded = self.rows_embedding_device(flat[2 * start:2 * stop], out=temporary[:2 * (stop - start)])
            _memb.dense_pair_similarity_to_device(index, decoded.data_ptr(), stop - start, dim, dim, *pointers(start, stop), stream)
        self._last_pairs_kernel = _memb.dense_pairs_kernel_name()
        return result

    def similarity_device(self, words_a, words_b):
        '''The cosine similarity of words_a[i] and words_b[i], a float32 (n,) tensor on the GPU: both lists resolved by
        resolve_rows_device, then pair_similarity_device. An unknown word gives 0.'''
        return self.pair_similarity_device(self.resolve_rows_device(words_a), self.resolve_rows_device(words_b))

    def pair_similarity(self, rows_a, rows_b, return_dots=False, return_norms=False):
        '''pair_similarity_device for host arrays: numpy row ids in, a numpy float32 (n,) array of cosines out, or
        (cosines, dots, norms) with either flag (None where not asked for). A reader on a GPU sends the ids up and brings
        the scalars back; a device='cpu' reader evaluates the same contract in numpy (pair_similarity_host) over
        rows_embedding in bounded slices: the same bits.'''
        rows_a = np.ascontiguousarray(rows_a, dtype=np.uint32).reshape(-1)
        rows_b = np.ascontiguousarray(rows_b, dtype=np.uint32).reshape(-1)
        if rows_a.size != rows_b.size:
            raise ValueError('rows_a and rows_b must have the same length')
        n = rows_a.size
        if self._impl.device() != _memb.HOST_DEVICE:
            import torch
            pairs = torch.from_numpy(np.stack((rows_a, rows_b), axis=1).view(np.int32)).to('cuda:{}'.format(self._impl.device()))
            result = self.pair_similarity_device(pairs, return_dots=return_dots, return_norms=return_norms)
            if return_dots or return_norms:
                return tuple(None if part is None else part.cpu().numpy() for part in result)
            return result.cpu().numpy()
        cosines = np.zeros(n, dtype=np.float32)
        dots = np.zeros(n, dtype=np.float32)
        norms = np.zeros((n, 2), dtype=np.float32)
        for start in range(0, n, NORMS_HOST_CHUNK):
            stop = start + NORMS_HOST_CHUNK
            cosines[start:stop], dots[start:stop], norms[start:stop] = pair_similarity_host(
                self.rows_embedding(rows_a[start:stop]), self.rows_embedding(rows_b[start:stop]))
        if return_dots or return_norms:
            return cosines, dots if return_dots else None, norms if return_norms else None
        return cosines

    @property
    def last_bag_pairs_kernel(self):
        """The kernel family of the last bag_pair_similarity_device call: 'bag_pairs_trained' (fused with the pooling) or
        'pairs_dense' behind a pooled lookup of the bags -- uniform and full storage, dims that are no multiple of 4 or
        beyond 512. '' before any call. Informational: the bits are the same."""
        return self._last_bag_pairs_kernel

    def bag_pair_similarity_device(self, rows, offsets, mode='mean', *, return_dots=False, return_norms=False, out=None):
        '''The cosine similarity of pairs of bags of rows, left on the GPU: a float32 (pairs,) tensor, cos[j] of the sums
        or means of the bags 2j and 2j + 1 -- the similarity of two sentences as averaged word vectors. For trained models
        whose dim is a multiple of 4 and at most 512 ONE kernel computes it from the compressed rows and writes no row;
        otherwise slices of whole pairs, of at most 2^20 bags, are pooled into a temporary (bags_embedding_device) and
        reduced there (last_bag_pairs_kernel says which). Bit for bit the contract of include/memb_hip_bag_pairs.h:
        pair_similarity_device's reduction over the rows bags_embedding_device(rows, offsets, mode) gives -- whichever
        kernel ran. Not clamped. A pair with an empty bag, or a bag of rows that are not in the model, has cosine 0.
        rows, offsets : as in bags_embedding_device; offsets holds 2 * pairs + 1 entries, an odd number (ValueError)
        mode : 'mean' or 'sum'
        return_dots, return_norms : either one returns (cosines, dots, norms) instead, dots a float32 (pairs,) and norms
            a float32 (pairs, 2) tensor -- row_norms_device's of the two pooled rows --, None where not asked for
        out : optional contiguous float32 (pairs,) tensor on the same device for the cosines
        One model, float32, missing='zero', the sequential order: no missing='skip', no reduction='chunked', no
        bfloat16 / float16, no ReadersUnion, no ShardedReader. One against many bags and the k nearest bags:
        bag_similarity_matrix_device, bag_similarity_topk_device.'''
        import torch
        code = pool_mode(mode)
        index, device = self._norms_arguments(torch, rows)
        if (not isinstance(offsets, torch.Tensor) or offsets.device.type != 'cuda' or offsets.dtype not in (torch.int32, torch.uint32)
                or not offsets.is_contiguous() or offsets.dim() != 1):
            raise TypeError('offsets must be a contiguous int32/uint32 tensor of 2 * pairs + 1 entries on the GPU')
        if offsets.numel() % 2 != 1:
            raise ValueError('offsets needs 2 * pairs + 1 entries, an odd number: pair j is the bags 2j and 2j + 1')
        n = offsets.numel() // 2
        if out is None:
            out = torch.empty((n,), dtype=torch.float32, device=device)
        if out.dtype != torch.float32 or out.dim() != 1 or out.shape[0] != n or not out.is_contiguous():
            raise TypeError('out must be a contiguous float32 (pairs,) tensor')
        if device.index != index or out.device != device or offsets.device != device:
            raise ValueError('rows, offsets and out must be on cuda:{} (the device this reader is staged on), got {}, {} and {}'.format(
                self.device, device, offsets.device, out.device))
        dots = torch.empty((n,), dtype=torch.float32, device=device) if return_dots else None
        norms = torch.empty((n, 2), dtype=torch.float32, device=device) if return_norms else None
        result = (out, dots, norms) if return_dots or return_norms else out

        def pointers(start, stop):
            return (out[start:stop].data_ptr(), dots[start:stop].data_ptr() if return_dots else 0,
                    norms[start:stop].data_ptr() if return_norms else 0)

        stream = _current_stream(torch, index)
        if self._impl.bag_pair_similarity_to_device(
                rows.data_ptr(), rows.numel(), offsets.data_ptr(), n, code, *pointers(0, n), stream):
            self._last_bag_pairs_kernel = self._impl.bag_pairs_kernel_name()
            return result
        flat = rows.reshape(-1)
        dim = self.dim
        slice_pairs = max(NORMS_DEVICE_SLICE // 2, 1)   # slices of at most NORMS_DEVICE_SLICE bags, an even number
        temporary = torch.empty((2 * min(n, slice_pairs), dim), dtype=torch.float32, device=device)
        for start in range(0, n, slice_pairs):
            stop = min(n, start + slice_pairs)
            entries, cut = flat, offsets
            if n > slice_pairs:
                # the slice's offsets as the kernel clamps them, rebased on the slice's lowest entry so that the pooled
                # launch is planned for the slice's entries alone: made on the device, with one scalar read back to cut
                # those entries out of `rows` (batches of more than 2^20 bags only)
                cut = offsets[2 * start:2 * stop + 1].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
                cut = torch.clamp(cut, max=flat.numel())
                first = int(cut.min())
                entries, cut = flat[first:], (cut - first).to(torch.int32)
            pooled = self.bags_embedding_device(entries, cut, mode=mode, out=temporary[:2 * (stop - start)])
            _memb.dense_pair_similarity_to_device(index, pooled.data_ptr(), stop - start, dim, dim, *pointers(start, stop), stream)
        self._last_bag_pairs_kernel = _memb.dense_pairs_kernel_name()
        return result

    def sentence_similarity_device(self, sentences_a, sentences_b, mode='mean'):
        '''The cosine similarity of sentences_a[i] and sentences_b[i] as pooled word vectors, a float32 (n,) tensor on the
        GPU: two equally long sequences of word sequences, interleaved, flattened (flatten_sentences), resolved on the
        device (resolve_rows_device) and reduced by bag_pair_similarity_device. An unknown word is a zero row that counts;
        a pair with a sentence without words gives 0.'''
        import torch
        pool_mode(mode)
        if len(sentences_a) != len(sentences_b):
            raise ValueError('sentences_a and sentences_b must have the same length')
        index = self._impl.device()
        if index == _memb.HOST_DEVICE:
            raise RuntimeError("this reader decodes on the host (device 'cpu'): device buffers need a reader on a HIP device")
        interleaved = [sentence for pair in zip(sentences_a, sentences_b) for sentence in pair]
        words, offsets = flatten_sentences(interleaved)
        device = 'cuda:{}'.format(index)
        rows = self.resolve_rows_device(words) if words else torch.empty((0,), dtype=torch.int32, device=device)
        on_device = torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).to(device)
        return self.bag_pair_similarity_device(rows, on_device, mode=mode)

    def bag_pair_similarity(self, rows, offsets, mode='mean', return_dots=False, return_norms=False):
        '''bag_pair_similarity_device for host arrays: numpy row ids and 2 * pairs + 1 offsets (bags_embedding's: ascending,
        within 0 .. len(rows)) in, a numpy float32 (pairs,) array of cosines out, or (cosines, dots, norms) with either
        flag (None where not asked for). A reader on a GPU sends the ids and offsets up and brings the scalars back; a
        device='cpu' reader evaluates the same contract in numpy (bags_embedding's sums, pair_similarity_host) in bounded
        slices: the same bits.'''
        code = pool_mode(mode)
        rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
        offsets = bag_offsets(offsets, rows.size)
        if offsets.size % 2 != 1:
            raise ValueError('offsets needs 2 * pairs + 1 entries, an odd number: pair j is the bags 2j and 2j + 1')
        n = offsets.size // 2
        if self._impl.device() != _memb.HOST_DEVICE:
            import torch
            device = 'cuda:{}'.format(self._impl.device())
            result = self.bag_pair_similarity_device(
                torch.from_numpy(rows.view(np.int32)).to(device),
                torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).to(device), mode=mode, return_dots=return_dots,
                return_norms=return_norms)
            if return_dots or return_norms:
                return tuple(None if part is None else part.cpu().numpy() for part in result)
            return result.cpu().numpy()
        cosines = np.zeros(n, dtype=np.float32)
        dots = np.zeros(n, dtype=np.float32)
        norms = np.zeros((n, 2), dtype=np.float32)
        slice_pairs = max(NORMS_HOST_CHUNK // 2, 1)
        for start in range(0, n, slice_pairs):
            stop = min(n, start + slice_pairs)
            cut = offsets[2 * start:2 * stop + 1]
            first, last = int(cut[0]), int(cut[-1])
            entries = rows[first:last]

            def slice_values(begin, end):
                yield self.rows_embedding(entries[begin:end])

            pooled, _ = pool_slices_host(
                cut - first, last - first, self.dim, BAGS_HOST_CHUNK, code == _memb.POOL_MEAN, False, slice_values)
            cosines[start:stop], dots[start:stop], norms[start:stop] = pair_similarity_host(pooled[0::2], pooled[1::2])
        if return_dots or return_norms:
            return cosines, dots if return_dots else None, norms if return_norms else None
        return cosines

    @property
    def last_query_kernel(self):
        '''The kernel family of the last query_similarity_device call: 'query_trained' (fused with the decode) or
        'pairs_dense' behind a plain decode of the candidates -- uniform and full storage, dims that are no multiple of 4
        or beyond 512. '' before any call. Informational: the bits are the same.'''
        return self._last_query_kernel

    def query_similarity_device(self, queries, rows, offsets=None, *, return_dots=False, return_norms=False, out=None):
        '''The cosine similarity of query vectors against groups of candidate rows, left on the GPU: a float32 (n,) tensor,
        cos[i] of query g and the row rows[i] for every entry i of group g -- one vector (a row, a difference of rows, a
        centroid, a pooled sentence) against a list of candidate words. For trained models whose dim is a multiple of 4 and
        at most 512 ONE kernel computes it from the compressed rows, a wavefront keeping its group's query in registers,
        and writes no row; otherwise slices of at most 2^19 candidates are decoded beside their queries into a temporary
        and reduced there (last_query_kernel says which). Bit for bit the contract of include/memb_hip_queries.h:
        pair_similarity_device's reduction over (query g, rows_embedding_device(rows)[i]) -- whichever kernel ran. Not
        clamped. A candidate that is not in the model has cosine 0. For the k best, torch.topk of the result.
        queries : float32 tensor of shape (G, dim), or (dim,) for one query, on this reader's device; rows may be strided
            (stride >= dim), the last dimension must be contiguous
        rows : as in rows_embedding_device, the n candidates of every group one after the other
        offsets : contiguous int32 / uint32 tensor of G + 1 ascending entries on the device, as in bags_embedding_device:
            group g owns the entries [min(offsets[g], n), min(offsets[g + 1], n)); None: one group of all rows (G == 1;
            the two offsets are copied to the device on the first call with that many rows and kept)
        return_dots, return_norms : either one returns (cosines, dots, norms) instead, dots a float32 (n,) tensor and norms
            the pair (query_norms (G,), row_norms (n,)) -- row_norms_device's of the candidates --, None where not asked for
        out : optional contiguous float32 (n,) tensor on the same device for the cosines; an entry that lies in no group is
            not written (it holds +0.0 in the tensors this method allocates)
        One model, float32: no top-k, no bfloat16 / float16, no ReadersUnion, no ShardedReader. Every query against ONE
        shared list, a (G, n) matrix, is similarity_matrix_device.'''
        import torch
        index, device = self._norms_arguments(torch, rows)
        dim = self.dim
        if not isinstance(queries, torch.Tensor) or queries.dtype != torch.float32:
            raise TypeError('queries must be a float32 tensor of shape (G, dim) or (dim,)')
        if queries.device.type != 'cuda':
            raise TypeError('queries must be on the GPU')
        if queries.dim() == 1:
            queries = queries.unsqueeze(0)
        if queries.dim() != 2 or queries.shape[1] != dim:
            raise ValueError('queries must have shape (G, {}) or ({},), got {}'.format(dim, dim, tuple(queries.shape)))
        groups = queries.shape[0]
        if (dim > 1 and queries.stride(1) != 1) or (groups > 1 and queries.stride(0) < dim):
            raise ValueError('queries must have a contiguous last dimension and a row stride of at least dim')
        ld = queries.stride(0) if groups > 1 else dim
        n = rows.numel()
        covered = offsets is None
        if covered:
            if groups != 1:
                raise ValueError('offsets=None means one group of all rows: queries must hold one query, got {}'.format(groups))
            # (kept from the last call with this many rows: repeated calls copy and allocate nothing)
            kept = self._whole_group_offsets
            if kept is None or kept[0] != (n, device):
                kept = ((n, device), torch.from_numpy(np.array([0, n], dtype=np.uint32).view(np.int32)).to(device))
                self._whole_group_offsets = kept
            offsets = kept[1]
        elif (not isinstance(offsets, torch.Tensor) or offsets.device.type != 'cuda' or offsets.dtype not in (torch.int32, torch.uint32)
                or not offsets.is_contiguous() or offsets.dim() != 1):
            raise TypeError('offsets must be a contiguous int32/uint32 tensor of G + 1 entries on the GPU')
        if offsets.numel() != groups + 1:
            raise ValueError('offsets needs G + 1 = {} entries, got {}'.format(groups + 1, offsets.numel()))
        allocate = torch.empty if covered else torch.zeros
        if out is None:
            out = allocate((n,), dtype=torch.float32, device=device)
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.dim() != 1 or out.shape[0] != n or not out.is_contiguous():
            raise TypeError('out must be a contiguous float32 (n,) tensor')
        if device.index != index or out.device != device or offsets.device != device or queries.device != device:
            raise ValueError('queries, rows, offsets and out must be on cuda:{} (the device this reader is staged on), got {}, {}, {} and {}'.format(
                self.device, queries.device, device, offsets.device, out.device))
        dots = allocate((n,), dtype=torch.float32, device=device) if return_dots else None
        row_norms = allocate((n,), dtype=torch.float32, device=device) if return_norms else None
        stream = _current_stream(torch, index)
        norms = None
        if return_norms:
            query_norms = torch.empty((groups,), dtype=torch.float32, device=device)
            if groups:
                _memb.dense_row_norms_to_device(index, queries.data_ptr(), groups, dim, ld, query_norms.data_ptr(), stream)
            norms = (query_norms, row_norms)
        result = (out, dots, norms) if return_dots or return_norms else out
        if n == 0 or groups == 0:   # (nothing to score: the C call would see three null outputs where n == 0)
            self._last_query_kernel = self._impl.query_kernel_name() or _memb.dense_pairs_kernel_name()
            return result
        if self._impl.query_similarity_to_device(
                queries.data_ptr(), groups, ld, rows.data_ptr(), n, offsets.data_ptr(), out.data_ptr(),
                dots.data_ptr() if return_dots else 0, row_norms.data_ptr() if return_norms else 0, stream):
            self._last_query_kernel = self._impl.query_kernel_name()
            return result
        self._last_query_kernel = _memb.dense_pairs_kernel_name()
        flat = rows.reshape(-1)
        # the entry-to-group map on the device: entry i lies in the last group whose clamped offset is <= i
        clamped = torch.clamp(offsets.view(torch.int32).to(torch.int64) & 0xFFFFFFFF, max=n)
        width = min(n, QUERY_DEVICE_SLICE)
        temporary = torch.empty((width, 2, dim), dtype=torch.float32, device=device)
        scalars = torch.empty((4, width), dtype=torch.float32, device=device)   # cosines, dots, the (width, 2) norms
        for start in range(0, n, QUERY_DEVICE_SLICE):
            stop = min(n, start + QUERY_DEVICE_SLICE)
            count = stop - start
            group = torch.searchsorted(clamped, torch.arange(start, stop, device=device), right=True) - 1
            inside = (group >= 0) & (group < groups)
            temporary[:count, 0] = queries[torch.clamp(group, 0, groups - 1)]
            self.rows_embedding_device(flat[start:stop], out=temporary.view(width, 2 * dim)[:count], col_off=dim)
            pair_norms = scalars[2:].reshape(-1)[:2 * count].view(count, 2)
            _memb.dense_pair_similarity_to_device(
                index, temporary.data_ptr(), count, dim, dim, scalars[0].data_ptr(), scalars[1].data_ptr(),
                pair_norms.data_ptr(), stream)
            for target, values in ((out, scalars[0, :count]), (dots, scalars[1, :count]), (row_norms, pair_norms[:, 1])):
                if target is not None:
                    target[start:stop] = torch.where(inside, values, target[start:stop])
        return result

    def candidates_similarity_device(self, words, candidate_lists):
        '''The cosine similarity of words[g] and each word of candidate_lists[g], on the GPU: (cosines, offsets), cosines a
        float32 (n,) tensor over the candidates of every list one after the other and offsets the int32 tensor of
        len(words) + 1 entries that says where each list begins among them. The query words and the flattened candidates
        (flatten_sentences) are resolved on the device (resolve_rows_device), the query rows decoded by
        rows_embedding_device, the rest is query_similarity_device. An unknown word -- query or candidate -- gives 0.'''
        import torch
        if len(words) != len(candidate_lists):
            raise ValueError('one list of candidates per word: got {} words and {} lists'.format(len(words), len(candidate_lists)))
        index = self._impl.device()
        if index == _memb.HOST_DEVICE:
            raise RuntimeError("this reader decodes on the host (device 'cpu'): device buffers need a reader on a HIP device")
        device = 'cuda:{}'.format(index)
        candidates, offsets = flatten_sentences(candidate_lists)
        on_device = torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).to(device)
        if not words:
            return torch.zeros((0,), dtype=torch.float32, device=device), on_device
        queries = self.rows_embedding_device(self.resolve_rows_device(list(words)))
        rows = self.resolve_rows_device(candidates) if candidates else torch.empty((0,), dtype=torch.int32, device=device)
        return self.query_similarity_device(queries, rows, on_device), on_device

    def query_similarity(self, queries, rows, offsets=None, return_dots=False, return_norms=False):
        '''query_similarity_device for host arrays: a numpy float32 (G, dim) or (dim,) array of queries, numpy row ids and
        G + 1 offsets (bags_embedding's: ascending, within 0 .. len(rows); None: one group of all rows) in, a numpy float32
        (n,) array of cosines out, or (cosines, dots, (query_norms, row_norms)) with either flag (None where not asked
        for). A reader on a GPU sends everything up and brings the scalars back; a device='cpu' reader evaluates the same
        contract in numpy (pair_similarity_host over rows_embedding) in bounded slices: the same bits. An entry that lies
        in no group is +0.0.'''
        queries = np.asarray(queries)
        if queries.dtype != np.float32:
            raise TypeError('queries must be a float32 array of shape (G, dim) or (dim,)')
        if queries.ndim == 1:
            queries = queries[None, :]
        if queries.ndim != 2 or queries.shape[1] != self.dim:
            raise ValueError('queries must have shape (G, {}) or ({},), got {}'.format(self.dim, self.dim, queries.shape))
        queries = np.ascontiguousarray(queries)
        groups = queries.shape[0]
        rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
        n = rows.size
        if offsets is None:
            if groups != 1:
                raise ValueError('offsets=None means one group of all rows: queries must hold one query, got {}'.format(groups))
            offsets = np.array([0, n], dtype=np.int64)
        offsets = bag_offsets(offsets, n)
        if offsets.size != groups + 1:
            raise ValueError('offsets needs G + 1 = {} entries, got {}'.format(groups + 1, offsets.size))
        if self._impl.device() != _memb.HOST_DEVICE:
            import torch
            device = 'cuda:{}'.format(self._impl.device())
            result = self.query_similarity_device(
                torch.from_numpy(queries).to(device), torch.from_numpy(rows.view(np.int32)).to(device),
                torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).to(device), return_dots=return_dots,
                return_norms=return_norms)
            if not (return_dots or return_norms):
                return result.cpu().numpy()
            cosines, dots, norms = result
            return (cosines.cpu().numpy(), None if dots is None else dots.cpu().numpy(),
                    None if norms is None else tuple(part.cpu().numpy() for part in norms))
        cosines = np.zeros(n, dtype=np.float32)
        dots = np.zeros(n, dtype=np.float32)
        row_norms = np.zeros(n, dtype=np.float32)
        group = np.searchsorted(offsets.astype(np.int64), np.arange(n, dtype=np.int64), side='right') - 1
        inside = (group >= 0) & (group < groups)
        for start in range(0, n, NORMS_HOST_CHUNK):
            chosen = start + np.flatnonzero(inside[start:start + NORMS_HOST_CHUNK])
            if chosen.size:
                cosines[chosen], dots[chosen], norms = pair_similarity_host(queries[group[chosen]], self.rows_embedding(rows[chosen]))
                row_norms[chosen] = norms[:, 1]
        if return_dots or return_norms:
            return (cosines, dots if return_dots else None,
                    (row_norms_host(queries) if groups else np.zeros(0, dtype=np.float32), row_norms) if return_norms else None)
        return cosines

    @property
    def last_query_matrix_kernel(self):
        '''The kernel family of the last similarity_matrix_device call: 'query_matrix_trained' (fused with the decode) or
        'pairs_dense' behind a plain decode of the candidates -- uniform and full storage, dims that are no multiple of 4
        or beyond 512. '' before any call. Informational: the bits are the same.'''
        return self._last_query_matrix_kernel

    def similarity_matrix_device(self, queries, rows, *, return_dots=False, return_norms=False, out=None):
        '''The cosine similarity of EVERY query vector against EVERY row of one shared candidate list, left on the GPU: a
        float32 (Q, n) tensor, cos[q, i] of query q and the row rows[i] -- a batch of analogy questions against the
        vocabulary, the neighbours of a few dozen words at once, a word-by-word matrix over a word list. For trained models
        whose dim is a multiple of 4 and at most 512 ONE kernel decodes every compressed row once, whatever Q is, scores it
        against all queries and writes no row; otherwise slices of at most 2^19 candidates are decoded once into a
        temporary and reduced there against one query after the other (last_query_matrix_kernel says which). Bit for bit
        the contract of include/memb_hip_query_matrix.h: row q is query_similarity_device(queries[q], rows) -- whichever
        kernel ran. Not clamped. A candidate that is not in the model has cosine 0. For the k best, torch.topk of the result.
        A matrix multiply over decoded rows is faster from some Q on, at other bits; this method never switches to it.
        queries : float32 tensor of shape (Q, dim), or (dim,) for one query, on this reader's device; rows may be strided
            (stride >= dim), the last dimension must be contiguous
        rows : as in rows_embedding_device, the n candidates every query shares
        return_dots, return_norms : either one returns (cosines, dots, norms) instead, dots a float32 (Q, n) tensor and norms
            the pair (query_norms (Q,), row_norms (n,)) -- row_norms_device's of the candidates --, None where not asked for
        out : optional float32 (Q, n) tensor on the same device for the cosines, with a contiguous last dimension and a row
            stride of at least n; nothing between its rows is written
        One model, float32: no top-k, no bfloat16 / float16, no ReadersUnion, no ShardedReader.'''
        import torch
        index, device = self._norms_arguments(torch, rows)
        dim = self.dim
        if not isinstance(queries, torch.Tensor) or queries.dtype != torch.float32:
            raise TypeError('queries must be a float32 tensor of shape (Q, dim) or (dim,)')
        if queries.device.type != 'cuda':
            raise TypeError('queries must be on the GPU')
        if queries.dim() == 1:
            queries = queries.unsqueeze(0)
        if queries.dim() != 2 or queries.shape[1] != dim:
            raise ValueError('queries must have shape (Q, {}) or ({},), got {}'.format(dim, dim, tuple(queries.shape)))
        count = queries.shape[0]
        if (dim > 1 and queries.stride(1) != 1) or (count > 1 and queries.stride(0) < dim):
            raise ValueError('queries must have a contiguous last dimension and a row stride of at least dim')
        ld = queries.stride(0) if count > 1 else dim
        n = rows.numel()
        if out is None:
            out = torch.empty((count, n), dtype=torch.float32, device=device)
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.dim() != 2 or tuple(out.shape) != (count, n):
            raise TypeError('out must be a float32 (Q, n) tensor')
        if (n > 1 and out.stride(1) != 1) or (count > 1 and out.stride(0) < n):
            raise ValueError('out must have a contiguous last dimension and a row stride of at least n')
        if device.index != index or out.device != device or queries.device != device:
            raise ValueError('queries, rows and out must be on cuda:{} (the device this reader is staged on), got {}, {} and {}'.format(
                self.device, queries.device, device, out.device))
        ld_out = out.stride(0) if count > 1 else n
        dots = torch.empty((count, n), dtype=torch.float32, device=device) if return_dots else None
        row_norms = torch.empty((n,), dtype=torch.float32, device=device) if return_norms else None
        stream = _current_stream(torch, index)
        norms = None
        if return_norms:
            query_norms = torch.empty((count,), dtype=torch.float32, device=device)
            if count:
                _memb.dense_row_norms_to_device(index, queries.data_ptr(), count, dim, ld, query_norms.data_ptr(), stream)
            norms = (query_norms, row_norms)
        result = (out, dots, norms) if return_dots or return_norms else out
        if n == 0:
            self._last_query_matrix_kernel = self._impl.query_matrix_kernel_name() or _memb.dense_pairs_kernel_name()
            return result
        if count == 0:   # (no query: the candidates' norms are all there is to work out)
            if return_norms:
                self.row_norms_device(rows.reshape(-1), out=row_norms)
            self._last_query_matrix_kernel = self._impl.query_matrix_kernel_name() or _memb.dense_pairs_kernel_name()
            return result
        if self._impl.query_matrix_to_device(
                queries.data_ptr(), count, ld, rows.data_ptr(), n, out.data_ptr(), dots.data_ptr() if return_dots else 0,
                ld_out, row_norms.data_ptr() if return_norms else 0, stream):
            self._last_query_matrix_kernel = self._impl.query_matrix_kernel_name()
            return result
        self._last_query_matrix_kernel = _memb.dense_pairs_kernel_name()
        flat = rows.reshape(-1)
        width = min(n, QUERY_DEVICE_SLICE)
        temporary = torch.empty((width, 2, dim), dtype=torch.float32, device=device)   # (query, decoded row) side by side
        pair_norms = torch.empty((width, 2), dtype=torch.float32, device=device)
        for start in range(0, n, QUERY_DEVICE_SLICE):
            stop = min(n, start + QUERY_DEVICE_SLICE)
            size = stop - start
            # the slice is decoded ONCE; every query is then written beside the same decoded rows
            self.rows_embedding_device(flat[start:stop], out=temporary.view(width, 2 * dim)[:size], col_off=dim)
            for q in range(count):
                temporary[:size, 0] = queries[q]
                _memb.dense_pair_similarity_to_device(
                    index, temporary.data_ptr(), size, dim, dim, out[q, start:stop].data_ptr(),
                    dots[q, start:stop].data_ptr() if return_dots else 0,
                    pair_norms.data_ptr() if return_norms and q == 0 else 0, stream)
                if return_norms and q == 0:
                    row_norms[start:stop] = pair_norms[:size, 1]
        return result

    def words_similarity_matrix_device(self, words_a, words_b):
        '''The cosine similarity of every word of words_a against every word of words_b, a float32
        (len(words_a), len(words_b)) tensor on the GPU: both lists resolved by resolve_rows_device, the rows of words_a
        decoded by rows_embedding_device as the queries, the rest is similarity_matrix_device. An unknown word -- on either
        side -- gives 0.'''
        import torch
        index = self._impl.device()
        if index == _memb.HOST_DEVICE:
            raise RuntimeError("this reader decodes on the host (device 'cpu'): device buffers need a reader on a HIP device")
        device = 'cuda:{}'.format(index)
        if not len(words_a) or not len(words_b):
            return torch.zeros((len(words_a), len(words_b)), dtype=torch.float32, device=device)
        queries = self.rows_embedding_device(self.resolve_rows_device(list(words_a)))
        return self.similarity_matrix_device(queries, self.resolve_rows_device(list(words_b)))

    def similarity_matrix(self, queries, rows, return_dots=False, return_norms=False):
        '''similarity_matrix_device for host arrays: a numpy float32 (Q, dim) or (dim,) array of queries and numpy row ids
        in, a numpy float32 (Q, n) array of cosines out, or (cosines, dots, (query_norms, row_norms)) with either flag (None
        where not asked for). A reader on a GPU sends everything up and brings the matrix back; a device='cpu' reader
        evaluates the same contract in numpy (pair_similarity_host over rows_embedding) in bounded slices, each slice
        decoded once for every query: the same bits.'''
        queries = np.asarray(queries)
        if queries.dtype != np.float32:
            raise TypeError('queries must be a float32 array of shape (Q, dim) or (dim,)')
        if queries.ndim == 1:
            queries = queries[None, :]
        if queries.ndim != 2 or queries.shape[1] != self.dim:
            raise ValueError('queries must have shape (Q, {}) or ({},), got {}'.format(self.dim, self.dim, queries.shape))
        queries = np.ascontiguousarray(queries)
        count = queries.shape[0]
        rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
        n = rows.size
        if self._impl.device() != _memb.HOST_DEVICE:
            import torch
            device = 'cuda:{}'.format(self._impl.device())
            result = self.similarity_matrix_device(
                torch.from_numpy(queries).to(device), torch.from_numpy(rows.view(np.int32)).to(device),
                return_dots=return_dots, return_norms=return_norms)
            if not (return_dots or return_norms):
                return result.cpu().numpy()
            cosines, dots, norms = result
            return (cosines.cpu().numpy(), None if dots is None else dots.cpu().numpy(),
                    None if norms is None else tuple(part.cpu().numpy() for part in norms))
        cosines = np.zeros((count, n), dtype=np.float32)
        dots = np.zeros((count, n), dtype=np.float32)
        row_norms = np.zeros(n, dtype=np.float32)
        for start in range(0, n, NORMS_HOST_CHUNK):
            values = self.rows_embedding(rows[start:start + NORMS_HOST_CHUNK])
            stop = start + len(values)
            row_norms[start:stop] = row_norms_host(values)
            for q in range(count):
                cosines[q, start:stop], dots[q, start:stop], _ = pair_similarity_host(np.broadcast_to(queries[q], values.shape), values)
        if return_dots or return_norms:
            return (cosines, dots if return_dots else None,
                    (row_norms_host(queries) if count else np.zeros(0, dtype=np.float32), row_norms) if return_norms else None)
        return cosines

    # ---- the k nearest candidates of every query (include/memb_hip_query_topk.h) ----

    @property
    def last_query_topk_kernel(self):
        '''The kernel families of the last similarity_topk_device call, joined by '+':
        'query_matrix_trained+topk_select+topk_merge' (slices of the fused matrix kernel in a workspace, selected there), or
        'pairs_dense+topk_select+topk_merge' where the matrix of a slice comes from similarity_matrix_device's fallback --
        uniform and full storage, dims that are no multiple of 4 or beyond 512; 'topk_merge' where such a model is asked
        with no candidate at all (the empty slots are all there is to write). '' before any call and after a call without
        queries, which launches nothing. Informational: the bits are the same.'''
        return self._last_query_topk_kernel

    def _topk_queries(self, torch, queries, index):
        """the checks of similarity_matrix_device on its queries: (queries as (Q, dim), Q, ld)"""
        dim = self.dim
        if not isinstance(queries, torch.Tensor) or queries.dtype != torch.float32:
            raise TypeError('queries must be a float32 tensor of shape (Q, dim) or (dim,)')
        if queries.device.type != 'cuda':
            raise TypeError('queries must be on the GPU')
        if queries.dim() == 1:
            queries = queries.unsqueeze(0)
        if queries.dim() != 2 or queries.shape[1] != dim:
            raise ValueError('queries must have shape (Q, {}) or ({},), got {}'.format(dim, dim, tuple(queries.shape)))
        count = queries.shape[0]
        if (dim > 1 and queries.stride(1) != 1) or (count > 1 and queries.stride(0) < dim):
            raise ValueError('queries must have a contiguous last dimension and a row stride of at least dim')
        if queries.device.index != index:
            raise ValueError('queries must be on cuda:{} (the device this reader is staged on), got {}'.format(index, queries.device))
        return queries, count, queries.stride(0) if count > 1 else dim

    def _all_rows_device(self, torch, index):
        """every row id of the model in order, on the device. Kept for the reader's lifetime once rows=None was asked for:
        4 bytes per word (8.8 MB for 2.2 M words), a torch tensor, so not part of info()['device_bytes']. Callers on other
        streams read it without an event of their own: it is built by one of them and finished before any other sees it."""
        rows = self._all_rows
        if rows is None or rows.device.index != index:
            with self._all_rows_lock:
                rows = self._all_rows
                if rows is None or rows.device.index != index:
                    rows = torch.arange(len(self), dtype=torch.int32, device='cuda:{}'.format(index))
                    if torch.cuda.is_current_stream_capturing():   # (a node of that graph: nothing to keep for others)
                        return rows
                    torch.cuda.current_stream(index).synchronize()
                    self._all_rows = rows
        return rows

    def _topk_exclude(self, torch, exclude, count, device):
        """the checks of similarity_topk_device on its exclusion list: (pointer, E, row stride in entries)"""
        if not isinstance(exclude, torch.Tensor) or exclude.dtype != torch.int64:
            raise TypeError('exclude must be an int64 tensor of shape (Q, E)')
        if exclude.device.type != 'cuda':
            raise TypeError('exclude must be on the GPU')
        if exclude.dim() != 2 or exclude.shape[0] != count:
            raise ValueError('exclude must have shape (Q, E) = ({}, E), got {}'.format(count, tuple(exclude.shape)))
        width = exclude.shape[1]
        if width > QUERY_TOPK_MAX_EXCLUDED:
            raise ValueError('exclude names at most {} positions per query, got {}'.format(QUERY_TOPK_MAX_EXCLUDED, width))
        if (width > 1 and exclude.stride(1) != 1) or (count > 1 and exclude.stride(0) < width):
            raise ValueError('exclude must have a contiguous last dimension and a row stride of at least E')
        if exclude.device != device:
            raise ValueError('exclude must be on {} (the device this reader is staged on), got {}'.format(device, exclude.device))
        return exclude.data_ptr() if width and count else 0, width, exclude.stride(0) if count > 1 else width

    def similarity_topk_device(self, queries, rows, k, *, workspace=None, exclude=None):
        '''The k most similar candidates of EVERY query, left on the GPU, WITHOUT the (Q, n) matrix of
        similarity_matrix_device in device memory: (values, positions), a float32 (Q, k) and an int64 (Q, k) tensor.
        Row q of similarity_matrix_device(queries, rows) ordered by a stable descending sort -- a greater cosine first, NaN
        before every number, equal cosines (-0.0 == +0.0) lower position first --, cut to k: positions[q, j] is the index
        into `rows` of the j-th best candidate and values[q, j] the matrix's bits there. Where n < k the last k - n
        entries are empty: position -1, value -inf (an empty slot is told by its position). The order is total, so this is
        torch.sort(matrix, dim=1, descending=True, stable=True) cut to k, whatever the slicing. For trained models whose dim
        is a multiple of 4 and at most 512 the matrix kernel fills a slice of the candidates in a workspace (about 32 MiB,
        independent of n) and two selection kernels merge it into the result; otherwise slices of at most 2^19 candidates
        go through similarity_matrix_device into one reused temporary and the same selection (last_query_topk_kernel says
        which).
        queries : as in similarity_matrix_device
        rows : as in rows_embedding_device, the n candidates every query shares; None: every row of the model in order, so
            positions are row ids (the ids are built on the device at the first such call and kept, 4 bytes per word,
            outside info()['device_bytes'])
        k : 1 .. 64 (QUERY_TOPK_MAX_K)
        workspace : optional contiguous uint8 tensor on the same device, aligned to 8 bytes, of at least
            self._impl.query_topk_workspace_bytes(Q, n, k, minimal=True) bytes, for the fused path: a call with it allocates
            nothing but its two results. Its size decides the slicing, never the result.
        exclude : optional int64 (Q, E) tensor on the same device, E <= 64 (QUERY_TOPK_MAX_EXCLUDED), with a contiguous last
            dimension and a row stride of at least E: positions (indices into `rows`) that are NO candidates of their query
            (include/memb_hip_analogies.h). Row q of the matrix without those columns is sorted and cut to k; the positions
            returned are still the original ones, and only n minus the distinct excluded positions can be filled. Entries
            may repeat and come in any order; a negative one or one beyond n is ignored (-1 pads a row). None: the call as
            it always was, the same kernels. With a list the selection kernel is topk_select_excluding
            (last_query_topk_kernel names it).
        One model, float32: no k > 64, no bfloat16 / float16, no ReadersUnion, no ShardedReader, no more than 64 exclusions.'''
        import torch
        index = self._impl.device()
        if index == _memb.HOST_DEVICE:
            raise RuntimeError("this reader decodes on the host (device 'cpu'): device buffers need a reader on a HIP device")
        k = topk_size(k)
        if rows is None:
            rows = self._all_rows_device(torch, index)
        self._norms_arguments(torch, rows)
        queries, count, ld = self._topk_queries(torch, queries, index)
        device = rows.device
        if device.index != index:
            raise ValueError('queries and rows must be on cuda:{} (the device this reader is staged on), got {} and {}'.format(
                self.device, queries.device, device))
        rows = rows.reshape(-1)
        n = rows.numel()
        values = torch.empty((count, k), dtype=torch.float32, device=device)
        positions = torch.empty((count, k), dtype=torch.int64, device=device)
        stream = _current_stream(torch, index)
        excluded = None if exclude is None else self._topk_exclude(torch, exclude, count, device)
        fused = self._impl.query_topk_kernel_name() if excluded is None else self._impl.query_topk_excluding_kernel_name()
        self._last_query_topk_kernel = fused if count else ''
        if count == 0:   # (nothing is launched)
            return values, positions
        if fused or n == 0:
            if not fused:   # (no candidate: topk_merge alone fills the empty slots, whatever the model)
                self._last_query_topk_kernel = 'topk_merge'
            if workspace is None:
                workspace = torch.empty((self._impl.query_topk_workspace_bytes(count, n, k),), dtype=torch.uint8, device=device)
            elif (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1
                    or not workspace.is_contiguous() or workspace.device != device):
                raise TypeError('workspace must be a contiguous uint8 tensor on cuda:{}'.format(index))
            if excluded is None:
                done = self._impl.query_topk_to_device(
                    queries.data_ptr(), count, ld, rows.data_ptr(), n, k, values.data_ptr(), positions.data_ptr(), k,
                    workspace.data_ptr() if workspace.numel() else 0, workspace.numel(), stream)
            else:
                done = self._impl.query_topk_excluding_to_device(
                    queries.data_ptr(), count, ld, rows.data_ptr(), n, k, *excluded, values.data_ptr(), positions.data_ptr(), k,
                    workspace.data_ptr() if workspace.numel() else 0, workspace.numel(), stream)
            assert done   # (n == 0 is answered for every model)
            return values, positions
        width = min(n, QUERY_DEVICE_SLICE)
        temporary = torch.empty((count, width), dtype=torch.float32, device=device)
        lists = torch.empty((topk_fallback_list_bytes(count, n, k, QUERY_DEVICE_SLICE),), dtype=torch.uint8, device=device)
        for start in range(0, n, QUERY_DEVICE_SLICE):
            size = min(n, start + QUERY_DEVICE_SLICE) - start
            self.similarity_matrix_device(queries, rows[start:start + size], out=temporary[:, :size])
            if excluded is None:
                _memb.dense_topk_to_device(
                    index, temporary.data_ptr(), count, size, width, start, k, start > 0, values.data_ptr(), positions.data_ptr(), k,
                    lists.data_ptr(), lists.numel(), stream)
            else:
                _memb.dense_topk_excluding_to_device(
                    index, temporary.data_ptr(), count, size, width, start, k, start > 0, *excluded, values.data_ptr(),
                    positions.data_ptr(), k, lists.data_ptr(), lists.numel(), stream)
        self._last_query_topk_kernel = self._last_query_matrix_kernel + '+' + (
            _memb.dense_topk_kernel_name() if excluded is None else _memb.dense_topk_excluding_kernel_name())
        return values, positions

    def most_similar_device(self, words, k=10, *, exclude_self=True):
        '''The k nearest words of each word over the WHOLE vocabulary, left on the GPU: (values, rows), a float32
        (len(words), k) tensor of cosines and an int64 (len(words), k) tensor of row ids (positions in keys()), best first
        in similarity_topk_device's order. The words are resolved and their rows decoded on the device, the rest is
        similarity_topk_device over every row. exclude_self: the word's own row is left out -- k + 1 are selected, the
        own row is dropped on the device, the rest keeps its order and its first k are returned --, so k <= 63. A repeated
        word gives repeated rows of output. A word that is not in the model gives a row of empty slots: row id -1, value
        -inf. No other exclusion list.'''
        import torch
        index = self._impl.device()
        if index == _memb.HOST_DEVICE:
            raise RuntimeError("this reader decodes on the host (device 'cpu'): device buffers need a reader on a HIP device")
        k = topk_size(k, 1 if exclude_self else 0)
        device = 'cuda:{}'.format(index)
        words = list(words)
        if not words:
            return torch.empty((0, k), dtype=torch.float32, device=device), torch.empty((0, k), dtype=torch.int64, device=device)
        own = self.resolve_rows_device(words)
        values, positions = self.similarity_topk_device(self.rows_embedding_device(own), None, k + 1 if exclude_self else k)
        own = own.to(torch.int64).unsqueeze(1)   # (a missing word is -1)
        if exclude_self:
            # stable: the entries that stay keep their order, the own row goes behind them
            order = torch.sort((positions == own).to(torch.int8), dim=1, stable=True).indices[:, :k]
            values, positions = torch.gather(values, 1, order), torch.gather(positions, 1, order)
        unknown = own < 0
        return (torch.where(unknown, torch.full_like(values, float('-inf')), values),
                torch.where(unknown, torch.full_like(positions, -1), positions))

    def most_similar(self, words, k=10):
        '''The k nearest words of each word over the whole vocabulary, on the host: one list of (word, cosine) pairs per
        word, best first, the word itself left out; [] for a word the model lacks. most_similar_device on a GPU reader,
        similarity_topk on a device='cpu' reader: the same pairs.'''
        words = list(words)
        k = topk_size(k, 1)
        if not words:
            return []
        if self._impl.device() != _memb.HOST_DEVICE:
            values, positions = (part.cpu().numpy() for part in self.most_similar_device(words, k))
        else:
            own = self.resolve_rows(words)
            values, positions = self.similarity_topk(self.rows_embedding(own), None, k + 1)
            order = np.argsort(positions == own.astype(np.int64)[:, None], axis=1, kind='stable')[:, :k]
            values, positions = np.take_along_axis(values, order, axis=1), np.take_along_axis(positions, order, axis=1)
            positions = np.where((own == 0xFFFFFFFF)[:, None], -1, positions)
        vocabulary = self.keys()
        return [[(vocabulary[row], float(value)) for value, row in zip(values[i], positions[i]) if row >= 0] for i in range(len(words))]

    def similarity_topk(self, queries, rows, k, exclude=None):
        '''similarity_topk_device for host arrays: a numpy float32 (Q, dim) or (dim,) array of queries and numpy row ids
        (None: every row of the model) in, (values float32 (Q, k), positions int64 (Q, k)) out. A reader on a GPU sends
        everything up and brings the result back; a device='cpu' reader takes similarity_matrix chunk by chunk and selects
        by the same order in numpy (topk_host): the same bits. exclude: similarity_topk_device's list as an integer (Q, E)
        array, E <= 64.'''
        queries = np.asarray(queries)
        if queries.dtype != np.float32:
            raise TypeError('queries must be a float32 array of shape (Q, dim) or (dim,)')
        if queries.ndim == 1:
            queries = queries[None, :]
        if queries.ndim != 2 or queries.shape[1] != self.dim:
            raise ValueError('queries must have shape (Q, {}) or ({},), got {}'.format(self.dim, self.dim, queries.shape))
        k = topk_size(k)
        queries = np.ascontiguousarray(queries)
        rows = np.arange(len(self), dtype=np.uint32) if rows is None else np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
        if exclude is not None:
            exclude = np.asarray(exclude)
            if exclude.dtype.kind not in 'iu':
                raise TypeError('exclude must be an integer array of shape (Q, E)')
            if exclude.ndim != 2 or exclude.shape[0] != queries.shape[0]:
                raise ValueError('exclude must have shape (Q, E) = ({}, E), got {}'.format(queries.shape[0], exclude.shape))
            if exclude.shape[1] > QUERY_TOPK_MAX_EXCLUDED:
                raise ValueError('exclude names at most {} positions per query, got {}'.format(QUERY_TOPK_MAX_EXCLUDED, exclude.shape[1]))
            exclude = np.ascontiguousarray(exclude, dtype=np.int64)
        if self._impl.device() != _memb.HOST_DEVICE:
            import torch
            device = 'cuda:{}'.format(self._impl.device())
            values, positions = self.similarity_topk_device(
                torch.from_numpy(queries).to(device), torch.from_numpy(rows.view(np.int32)).to(device), k,
                exclude=None if exclude is None else torch.from_numpy(exclude).to(device))
            return values.cpu().numpy(), positions.cpu().numpy()
        values = np.full((queries.shape[0], k), -np.inf, dtype=np.float32)
        positions = np.full((queries.shape[0], k), -1, dtype=np.int64)
        for start in range(0, rows.size, NORMS_HOST_CHUNK):
            matrix = self.similarity_matrix(queries, rows[start:start + NORMS_HOST_CHUNK])
            values, positions = topk_host(matrix, k, start, (values, positions), exclude)
        return values, positions

    # ---- analogies: signed word queries and the top-k without their own words (include/memb_hip_analogies.h) ----

    def compose_queries_device(self, rows, offsets, weights=None):
        '''Query vectors built from several rows each, left on the GPU: a float32 (Q, dim) tensor. Query q is the sum over
        the entries offsets[q] .. offsets[q + 1] of weights[e] * unit row of rows[e], added in entry order from +0.0, the
        product and the sum each one float32 operation (include/memb_hip_analogies.h) -- so the bits are the same on every
        path, which a segmented sum in torch (index_add_) does not promise. The unit rows are
        unit_rows_embedding_device(rows) in a temporary of (entries, dim) floats, summed by one more kernel
        (weighted_rows_sum): not fused with the decode. A row that is not in the model is a zero row; a query without
        entries is +0.0.
        rows : as in rows_embedding_device, the entries of all queries
        offsets : contiguous int32 / uint32 tensor of Q + 1 ascending entries on the same device; an offset beyond
            len(rows) is clamped to it
        weights : optional contiguous float32 tensor of len(rows) entries on the same device; None: all +1'''
        import torch
        index, device = self._norms_arguments(torch, rows)
        count = self._bag_arguments(torch, rows, offsets, index, device)
        rows = rows.reshape(-1)
        n = rows.numel()
        if weights is not None:
            if (not isinstance(weights, torch.Tensor) or weights.dtype != torch.float32 or weights.device != device
                    or not weights.is_contiguous() or weights.numel() != n):
                raise TypeError('weights must be a contiguous float32 tensor of len(rows) entries on {}'.format(device))
        dim = self.dim
        unit = self.unit_rows_embedding_device(rows) if n else None
        # (the kernel trusts its offsets: none may point past the unit rows)
        offsets = torch.clamp(offsets.view(torch.int32).to(torch.int64) & 0xFFFFFFFF, max=n).to(torch.int32)
        out = torch.empty((count, dim), dtype=torch.float32, device=device)
        _memb.weighted_rows_sum_to_device(
            index, unit.data_ptr() if n else 0, dim, weights.data_ptr() if n and weights is not None else 0, offsets.data_ptr(),
            count, dim, out.data_ptr(), dim, _current_stream(torch, index))
        return out

    def compose_queries(self, rows, offsets, weights=None):
        '''compose_queries_device for host arrays: numpy row ids, offsets (Q + 1 ascending integers within 0 .. len(rows))
        and optional float32 weights in, a numpy float32 (Q, dim) matrix out. A reader on a GPU sends everything up and
        brings the queries back; a device='cpu' reader adds its unit_rows_embedding in numpy in the same order
        (weighted_rows_sum_host): the same bits.'''
        rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
        offsets = bag_offsets(offsets, rows.size)
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=np.float32).reshape(-1)
            if weights.size != rows.size:
                raise ValueError('weights needs one entry per row, got {} for {}'.format(weights.size, rows.size))
        if self._impl.device() != _memb.HOST_DEVICE:
            import torch
            device = 'cuda:{}'.format(self._impl.device())
            return self.compose_queries_device(
                torch.from_numpy(rows.view(np.int32)).to(device), torch.from_numpy(offsets.astype(np.int32)).to(device),
                None if weights is None else torch.from_numpy(weights).to(device)).cpu().numpy()
        return weighted_rows_sum_host(self.unit_rows_embedding(rows), weights, offsets)

    @staticmethod
    def _analogy_entries(positive, negative):
        """The entries of analogies: (words, weights float32, offsets int64 (Q + 1), members int64 (Q, E)) -- per query its
        positive entries, then its negative ones, each in the order given, a bare word weighing +1 among the positive and
        -1 among the negative; members[q]: the indices of query q's entries in `words`, -1 behind them."""
        positive = [list(entries) for entries in positive]
        negative = [[] for _ in positive] if negative is None else [list(entries) for entries in negative]
        if len(negative) != len(positive):
            raise ValueError('positive and negative must hold one list per query, got {} and {}'.format(len(positive), len(negative)))
        words, weights, offsets = [], [], [0]
        for plus, minus in zip(positive, negative):
            for entries, default in ((plus, 1.0), (minus, -1.0)):
                for entry in entries:
                    word, weight = (entry, default) if isinstance(entry, (str, bytes)) else entry
                    words.append(word)
                    weights.append(weight)
            if len(words) - offsets[-1] > QUERY_TOPK_MAX_EXCLUDED:
                raise ValueError('a query takes at most {} words (each is excluded from its answer), got {}'.format(
                    QUERY_TOPK_MAX_EXCLUDED, len(words) - offsets[-1]))
            offsets.append(len(words))
        offsets = np.array(offsets, dtype=np.int64)
        lengths = offsets[1:] - offsets[:-1]
        width = int(lengths.max()) if lengths.size else 0
        steps = np.arange(width, dtype=np.int64)[None, :]
        members = np.where(steps < lengths[:, None], offsets[:-1, None] + steps, -1)
        return words, np.array(weights, dtype=np.float32), offsets, members

    def analogies_device(self, positive, negative=None, k=10):
        '''The k nearest words of signed word queries over the WHOLE vocabulary, left on the GPU -- king - man + woman is
        positive=[['king', 'woman']], negative=[['man']], gensim's most_similar(positive=, negative=): (values, rows), a
        float32 (Q, k) tensor of cosines and an int64 (Q, k) tensor of row ids (positions in keys()), best first in
        similarity_topk_device's order.
        positive, negative : one list per query of words or (word, weight) pairs; a bare word weighs +1 in positive and -1
            in negative. negative=None: no negative words. At most 64 words per query (ValueError beyond).
        The query is compose_queries_device over a query's positive entries, then its negative ones, each in the order
        given: the sum of weighted UNIT rows, which is gensim's query up to a scale the cosine does not see. The candidates
        are every row of the model, and the rows of ALL of a query's words are excluded (similarity_topk_device's exclude),
        so no input word appears in its answer and none costs a rank: k goes up to 64. A query with a word the model lacks,
        or without any word, gives a row of empty slots: row id -1, value -inf. Cosine addition only: 3CosMul is
        analogies_cosmul_device.'''
        import torch
        index = self._impl.device()
        if index == _memb.HOST_DEVICE:
            raise RuntimeError("this reader decodes on the host (device 'cpu'): device buffers need a reader on a HIP device")
        k = topk_size(k)
        device = 'cuda:{}'.format(index)
        words, weights, offsets, members = self._analogy_entries(positive, negative)
        count = offsets.size - 1
        if count == 0:
            return torch.empty((0, k), dtype=torch.float32, device=device), torch.empty((0, k), dtype=torch.int64, device=device)
        own = self.resolve_rows_device(words)
        queries = self.compose_queries_device(
            own, torch.from_numpy(offsets.astype(np.int32)).to(device), torch.from_numpy(weights).to(device))
        members = torch.from_numpy(members).to(device)
        padded = torch.cat([own.to(torch.int64), torch.full((1,), -1, dtype=torch.int64, device=device)])   # (a missing word is -1)
        exclude = padded[members]   # (members == -1 reads the -1 at the end)
        values, positions = self.similarity_topk_device(queries, None, k, exclude=exclude)
        unanswered = ((members >= 0) & (exclude < 0)).any(dim=1) | torch.from_numpy(offsets[1:] == offsets[:-1]).to(device)
        unanswered = unanswered.unsqueeze(1)
        return (torch.where(unanswered, torch.full_like(values, float('-inf')), values),
                torch.where(unanswered, torch.full_like(positions, -1), positions))

    def analogies(self, positive, negative=None, k=10):
        '''analogies_device on the host: one list of (word, cosine) pairs per query, best first, none of the query's own
        words among them; [] for a query with a word the model lacks or without any word. analogies_device on a GPU reader;
        compose_queries and similarity_topk with the same exclusion on a device='cpu' reader: the same pairs.'''
        k = topk_size(k)
        if self._impl.device() != _memb.HOST_DEVICE:
            values, positions = (part.cpu().numpy() for part in self.analogies_device(positive, negative, k))
        else:
            words, weights, offsets, members = self._analogy_entries(positive, negative)
            if offsets.size == 1:
                return []
            own = self.resolve_rows(words)
            rows = np.concatenate([np.where(own == 0xFFFFFFFF, -1, own.astype(np.int64)), [-1]])
            exclude = rows[members]
            values, positions = self.similarity_topk(self.compose_queries(own, offsets, weights), None, k, exclude=exclude)
            unanswered = ((members >= 0) & (exclude < 0)).any(axis=1) | (offsets[1:] == offsets[:-1])
            positions = np.where(unanswered[:, None], -1, positions)
        vocabulary = self.keys()
        return [[(vocabulary[row], float(value)) for value, row in zip(values[i], positions[i]) if row >= 0]
                for i in range(values.shape[0])]

    def analogy(self, a, b, c, k=1):
        '''a is to b as c is to ...: the k nearest words of b - a + c as (word, cosine) pairs, a, b and c left out;
        analogies([[b, c]], [[a]], k)[0].'''
        return self.analogies([[b, c]], [[a]], k)[0]

    # ---- 3CosMul: the multiplicative analogy score and the top-k by it (include/memb_hip_cosmul.h) ----

    @property
    def last_cosmul_kernel(self):
        '''The kernel families of the last cosmul_topk_device call, joined by '+':
        'query_matrix_trained+cosmul_scores+topk_select_excluding+topk_merge' (slices of the fused matrix kernel in a
        workspace, scored and selected there), or 'pairs_dense+cosmul_scores+topk_select_excluding+topk_merge' where the
        cosines of a slice come from similarity_matrix_device's fallback -- uniform and full storage, dims that are no
        multiple of 4 or beyond 512; 'topk_merge' where such a model is asked with no candidate at all. '' before any call
        and after a call without questions, which launches nothing. Informational: the bits are the same.'''
        return self._last_cosmul_kernel

    def cosmul_topk_device(self, terms, offsets, negatives_from, rows, k, *, exclude=None, workspace=None, questions=None):
        '''The k best candidates of EVERY question by the 3CosMul score (Levy & Goldberg; gensim's most_similar_cosmul),
        left on the GPU, without the (T, n) matrix of cosines or the (Q, n) matrix of scores in device memory: (values,
        positions), a float32 (Q, k) and an int64 (Q, k) tensor in similarity_topk_device's order and with its empty slots.
        For a candidate with the cosines c of similarity_matrix_device(terms, rows) against a question's terms:
        num = product of (1 + c) * 0.5 over its positive terms, den likewise over its negative ones, score = num / (den +
        1e-6), every operation one float32 operation in the order of the terms (include/memb_hip_cosmul.h), so the bits
        are the same on every path. For trained models whose dim is a multiple of 4 and at most 512 the matrix kernel
        fills a slice of the candidates in a workspace, cosmul_scores turns it into scores and two selection kernels merge
        them into the result; otherwise slices of at most 2^19 candidates go through similarity_matrix_device,
        cosmul_scores and the same selection (last_cosmul_kernel says which).
        terms : float32 (T, dim) tensor on this reader's device, as the queries of similarity_matrix_device
        offsets : Q + 1 ascending host integers within 0 .. T: question q takes the terms offsets[q] .. offsets[q + 1], at
            most 64 (COSMUL_MAX_TERMS) of them
        negatives_from : Q host integers, offsets[q] <= negatives_from[q] <= offsets[q + 1]: the terms before it are
            positive, those from it on negative. Both arrays are checked on the host (ValueError) and uploaded by the call.
        rows : as in similarity_topk_device; None: every row of the model in order
        k : 1 .. 64
        exclude : as in similarity_topk_device, one row per question
        workspace : optional contiguous uint8 tensor on the same device, aligned to 8 bytes, of at least
            _memb_cosmul.query_cosmul_workspace_bytes(self._impl.context_handle(), T, Q, n, k, minimal=True) bytes, for the
            fused path. Its size decides the slicing, never the result.
        questions : optional contiguous int32 tensor of 2 Q + 1 entries on the same device: offsets, then negatives_from, as
            the call uploads them where it is None. That upload is a copy from the host, which no graph capture admits: a
            caller who captures the call uploads the tensor beforehand, keeps it alive for the replays and passes it here.
            offsets and negatives_from are given and checked all the same, and the tensor must hold their numbers (the
            kernels trust it).
        One model, float32: no weights, no k > 64, no more than 64 terms, no bfloat16 / float16, no ReadersUnion, no
        ShardedReader, no pooled-bag candidates.'''
        import torch
        index = self._impl.device()
        if index == _memb.HOST_DEVICE:
            raise RuntimeError("this reader decodes on the host (device 'cpu'): device buffers need a reader on a HIP device")
        k = topk_size(k)
        if rows is None:
            rows = self._all_rows_device(torch, index)
        self._norms_arguments(torch, rows)
        if isinstance(terms, torch.Tensor) and terms.dim() != 2:
            raise ValueError('terms must have shape (T, {}), got {}'.format(self.dim, tuple(terms.shape)))
        terms, n_terms, ld = self._topk_queries(torch, terms, index)
        offsets, negatives_from = cosmul_questions(offsets, negatives_from, n_terms)
        count = negatives_from.size
        device = rows.device
        if device.index != index:
            raise ValueError('terms and rows must be on cuda:{} (the device this reader is staged on), got {} and {}'.format(
                self.device, terms.device, device))
        rows = rows.reshape(-1)
        n = rows.numel()
        values = torch.empty((count, k), dtype=torch.float32, device=device)
        positions = torch.empty((count, k), dtype=torch.int64, device=device)
        stream = _current_stream(torch, index)
        excluded = (0, 0, 0) if exclude is None else self._topk_exclude(torch, exclude, count, device)
        context = self._impl.context_handle()
        fused = _memb_cosmul.query_cosmul_kernel_name(context)
        self._last_cosmul_kernel = fused if count else ''
        if count == 0:   # (nothing is launched)
            return values, positions
        if questions is None:
            questions = torch.from_numpy(np.concatenate([offsets, negatives_from]).astype(np.int32)).to(device)
        elif (not isinstance(questions, torch.Tensor) or questions.dtype != torch.int32 or questions.dim() != 1
                or not questions.is_contiguous() or questions.device != device or questions.numel() != 2 * count + 1):
            raise TypeError('questions must be a contiguous int32 tensor of 2 Q + 1 = {} entries on cuda:{}'.format(2 * count + 1, index))
        offsets_ptr, negatives_ptr = questions.data_ptr(), questions[count + 1:].data_ptr() if count else 0
        if fused or n == 0:
            if not fused:   # (no candidate: topk_merge alone fills the empty slots, whatever the model)
                self._last_cosmul_kernel = 'topk_merge'
            if workspace is None:
                workspace = torch.empty((_memb_cosmul.query_cosmul_workspace_bytes(context, n_terms, count, n, k),), dtype=torch.uint8, device=device)
            elif (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1
                    or not workspace.is_contiguous() or workspace.device != device):
                raise TypeError('workspace must be a contiguous uint8 tensor on cuda:{}'.format(index))
            done = _memb_cosmul.query_cosmul_nearest_to_device(
                context, terms.data_ptr(), n_terms, ld, offsets_ptr, negatives_ptr, count, rows.data_ptr(), n, k, *excluded,
                values.data_ptr(), positions.data_ptr(), k, workspace.data_ptr() if workspace.numel() else 0, workspace.numel(),
                stream)
            assert done   # (n == 0 is answered for every model)
            return values, positions
        width = min(n, QUERY_DEVICE_SLICE)
        cosines = torch.empty((max(n_terms, 1), width), dtype=torch.float32, device=device)   # (a row where no term exists: a pointer to hand over)
        scores = torch.empty((count, width), dtype=torch.float32, device=device)
        lists = torch.empty((topk_fallback_list_bytes(count, n, k, QUERY_DEVICE_SLICE),), dtype=torch.uint8, device=device)
        for start in range(0, n, QUERY_DEVICE_SLICE):
            size = min(n, start + QUERY_DEVICE_SLICE) - start
            if n_terms:
                self.similarity_matrix_device(terms, rows[start:start + size], out=cosines[:n_terms, :size])
            _memb_cosmul.cosmul_scores_to_device(
                index, cosines.data_ptr(), width, offsets_ptr, negatives_ptr, count, size, scores.data_ptr(), width, stream)
            _memb.dense_topk_excluding_to_device(
                index, scores.data_ptr(), count, size, width, start, k, start > 0, *excluded, values.data_ptr(),
                positions.data_ptr(), k, lists.data_ptr(), lists.numel(), stream)
        matrix = self._last_query_matrix_kernel if n_terms else ''
        self._last_cosmul_kernel = '+'.join(
            part for part in (matrix, _memb_cosmul.cosmul_scores_kernel_name(), _memb.dense_topk_excluding_kernel_name()) if part)
        return values, positions

    def cosmul_topk(self, terms, offsets, negatives_from, rows, k, exclude=None):
        '''cosmul_topk_device for host arrays: a numpy float32 (T, dim) array of terms, the questions and numpy row ids (None:
        every row of the model) in, (values float32 (Q, k), positions int64 (Q, k)) out. A reader on a GPU sends everything
        up and brings the result back; a device='cpu' reader takes similarity_matrix chunk by chunk, scores it in numpy
        (cosmul_scores_host) and selects by the same order (topk_host): the same bits. exclude: an integer (Q, E) array,
        E <= 64.'''
        terms = np.asarray(terms)
        if terms.dtype != np.float32:
            raise TypeError('terms must be a float32 array of shape (T, dim)')
        if terms.ndim != 2 or terms.shape[1] != self.dim:
            raise ValueError('terms must have shape (T, {}), got {}'.format(self.dim, terms.shape))
        k = topk_size(k)
        terms = np.ascontiguousarray(terms)
        offsets, negatives_from = cosmul_questions(offsets, negatives_from, terms.shape[0])
        count = negatives_from.size
        rows = np.arange(len(self), dtype=np.uint32) if rows is None else np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
        if exclude is not None:
            exclude = np.asarray(exclude)
            if exclude.dtype.kind not in 'iu':
                raise TypeError('exclude must be an integer array of shape (Q, E)')
            if exclude.ndim != 2 or exclude.shape[0] != count:
                raise ValueError('exclude must have shape (Q, E) = ({}, E), got {}'.format(count, exclude.shape))
            if exclude.shape[1] > QUERY_TOPK_MAX_EXCLUDED:
                raise ValueError('exclude names at most {} positions per query, got {}'.format(QUERY_TOPK_MAX_EXCLUDED, exclude.shape[1]))
            exclude = np.ascontiguousarray(exclude, dtype=np.int64)
        if self._impl.device() != _memb.HOST_DEVICE:
            import torch
            device = 'cuda:{}'.format(self._impl.device())
            values, positions = self.cosmul_topk_device(
                torch.from_numpy(terms).to(device), offsets, negatives_from, torch.from_numpy(rows.view(np.int32)).to(device), k,
                exclude=None if exclude is None else torch.from_numpy(exclude).to(device))
            return values.cpu().numpy(), positions.cpu().numpy()
        values = np.full((count, k), -np.inf, dtype=np.float32)
        positions = np.full((count, k), -1, dtype=np.int64)
        for start in range(0, rows.size, NORMS_HOST_CHUNK):
            scores = cosmul_scores_host(self.similarity_matrix(terms, rows[start:start + NORMS_HOST_CHUNK]), offsets, negatives_from)
            values, positions = topk_host(scores, k, start, (values, positions), exclude)
        return values, positions

    @staticmethod
    def _cosmul_entries(positive, negative):
        '''The entries of analogies_cosmul: (words, offsets int64 (Q + 1), negatives_from int64 (Q), members int64 (Q, E)) --
        per question its positive words, then its negative ones, each in the order given; members as in _analogy_entries.'''
        positive = [list(entries) for entries in positive]
        negative = [[] for _ in positive] if negative is None else [list(entries) for entries in negative]
        if len(negative) != len(positive):
            raise ValueError('positive and negative must hold one list per query, got {} and {}'.format(len(positive), len(negative)))
        words, offsets, negatives_from = [], [0], []
        for plus, minus in zip(positive, negative):
            for entry in plus + minus:
                if not isinstance(entry, (str, bytes)):
                    raise TypeError('3CosMul takes bare words: it has no weights, got {!r}'.format(entry))
            words.extend(plus)
            negatives_from.append(len(words))
            words.extend(minus)
            if len(words) - offsets[-1] > COSMUL_MAX_TERMS:
                raise ValueError('a question takes at most {} words (each is excluded from its answer), got {}'.format(
                    COSMUL_MAX_TERMS, len(words) - offsets[-1]))
            offsets.append(len(words))
        offsets = np.array(offsets, dtype=np.int64)
        lengths = offsets[1:] - offsets[:-1]
        width = int(lengths.max()) if lengths.size else 0
        steps = np.arange(width, dtype=np.int64)[None, :]
        members = np.where(steps < lengths[:, None], offsets[:-1, None] + steps, -1)
        return words, offsets, np.array(negatives_from, dtype=np.int64), members

    def analogies_cosmul_device(self, positive, negative=None, k=10):
        '''analogies_device by the 3CosMul score instead of the cosine of a summed query -- gensim's
        most_similar_cosmul(positive=, negative=) -- over the WHOLE vocabulary, left on the GPU: (values, rows), a float32
        (Q, k) tensor of scores and an int64 (Q, k) tensor of row ids (positions in keys()), best first.
        positive, negative : one list of bare words per question; a (word, weight) pair is a TypeError, since 3CosMul has no
            weights. negative=None: no negative words. At most 64 words per question (ValueError beyond).
        The terms are unit_rows_embedding_device of the resolved words, the rest is cosmul_topk_device over every row of the
        model with the rows of ALL of a question's words excluded, so k goes up to 64. A question with a word the model
        lacks, or without any word, gives a row of empty slots: row id -1, value -inf.'''
        import torch
        index = self._impl.device()
        if index == _memb.HOST_DEVICE:
            raise RuntimeError("this reader decodes on the host (device 'cpu'): device buffers need a reader on a HIP device")
        k = topk_size(k)
        device = 'cuda:{}'.format(index)
        words, offsets, negatives_from, members = self._cosmul_entries(positive, negative)
        count = offsets.size - 1
        if count == 0:
            return torch.empty((0, k), dtype=torch.float32, device=device), torch.empty((0, k), dtype=torch.int64, device=device)
        if words:
            own = self.resolve_rows_device(words)
            terms = self.unit_rows_embedding_device(own)
        else:
            own = torch.empty((0,), dtype=torch.int32, device=device)
            terms = torch.empty((0, self.dim), dtype=torch.float32, device=device)
        members = torch.from_numpy(members).to(device)
        padded = torch.cat([own.to(torch.int64), torch.full((1,), -1, dtype=torch.int64, device=device)])   # (a missing word is -1)
        exclude = padded[members]   # (members == -1 reads the -1 at the end)
        values, positions = self.cosmul_topk_device(terms, offsets, negatives_from, None, k, exclude=exclude)
        unanswered = ((members >= 0) & (exclude < 0)).any(dim=1) | torch.from_numpy(offsets[1:] == offsets[:-1]).to(device)
        unanswered = unanswered.unsqueeze(1)
        return (torch.where(unanswered, torch.full_like(values, float('-inf')), values),
                torch.where(unanswered, torch.full_like(positions, -1), positions))

    def analogies_cosmul(self, positive, negative=None, k=10):
        '''analogies_cosmul_device on the host: one list of (word, score) pairs per question, best first, none of the
        question's own words among them; [] for a question with a word the model lacks or without any word.
        analogies_cosmul_device on a GPU reader; unit_rows_embedding and cosmul_topk with the same exclusion on a
        device='cpu' reader: the same pairs.'''
        k = topk_size(k)
        if self._impl.device() != _memb.HOST_DEVICE:
            values, positions = (part.cpu().numpy() for part in self.analogies_cosmul_device(positive, negative, k))
        else:
            words, offsets, negatives_from, members = self._cosmul_entries(positive, negative)
            if offsets.size == 1:
                return []
            own = self.resolve_rows(words) if words else np.zeros(0, dtype=np.uint32)
            terms = self.unit_rows_embedding(own) if words else np.zeros((0, self.dim), dtype=np.float32)
            rows = np.concatenate([np.where(own == 0xFFFFFFFF, -1, own.astype(np.int64)), [-1]])
            exclude = rows[members]
            values, positions = self.cosmul_topk(terms, offsets, negatives_from, None, k, exclude=exclude)
            unanswered = ((members >= 0) & (exclude < 0)).any(axis=1) | (offsets[1:] == offsets[:-1])
            positions = np.where(unanswered[:, None], -1, positions)
        vocabulary = self.keys()
        return [[(vocabulary[row], float(value)) for value, row in zip(values[i], positions[i]) if row >= 0]
                for i in range(values.shape[0])]

    def analogy_cosmul(self, a, b, c, k=1):
        '''a is to b as c is to ... by 3CosMul: the k best words as (word, score) pairs, a, b and c left out;
        analogies_cosmul([[b, c]], [[a]], k)[0].'''
        return self.analogies_cosmul([[b, c]], [[a]], k)[0]

    # ---- the rank of a given candidate: how many candidates precede a mark (include/memb_hip_ranks.h) ----

    @property
    def last_ranks_kernel(self):
        '''The kernel families of the last similarity_ranks_device call, joined by '+':
        'query_matrix_trained+rank_count+rank_fold' (slices of the fused matrix kernel in a workspace, counted there), or
        'pairs_dense+rank_count+rank_fold' where the cosines of a slice come from similarity_matrix_device's fallback --
        uniform and full storage, dims that are no multiple of 4 or beyond 512; 'rank_fold' where such a model is asked
        with no candidate at all. '' before any call and after a call without queries, which launches nothing.
        Informational: the counts are the same.'''
        return self._last_ranks_kernel

    def _marks_arguments(self, torch, queries, rows, thresholds, marks, exclude):
        """the checks similarity_ranks_device and similarity_within_device share, before anything is launched: (index,
        queries as (Q, dim), Q, ld, rows flattened, n, device, the list of non-candidates as (pointer, E, row stride))"""
        index = self._impl.device()
        if index == _memb.HOST_DEVICE:
            raise RuntimeError("this reader decodes on the host (device 'cpu'): device buffers need a reader on a HIP device")
        if rows is None:
            rows = self._all_rows_device(torch, index)
        self._norms_arguments(torch, rows)
        queries, count, ld = self._topk_queries(torch, queries, index)
        device = rows.device
        if device.index != index:
            raise ValueError('queries and rows must be on cuda:{} (the device this reader is staged on), got {} and {}'.format(
                self.device, queries.device, device))
        for name, tensor, dtype in (('thresholds', thresholds, torch.float32), ('marks', marks, torch.int64)):
            if tensor is None and name == 'marks':
                continue
            if not isinstance(tensor, torch.Tensor) or tensor.dtype != dtype:
                raise TypeError('{} must be a {} tensor of shape (Q,)'.format(name, 'float32' if dtype == torch.float32 else 'int64'))
            if tensor.device.type != 'cuda':
                raise TypeError('{} must be on the GPU'.format(name))
            if tensor.dim() != 1 or tensor.shape[0] != count or not tensor.is_contiguous():
                raise ValueError('{} must be contiguous with shape (Q,) = ({},), got {}'.format(name, count, tuple(tensor.shape)))
            if tensor.device != device:
                raise ValueError('{} must be on {} (the device this reader is staged on), got {}'.format(name, device, tensor.device))
        excluded = (0, 0, 0) if exclude is None else self._topk_exclude(torch, exclude, count, device)
        rows = rows.reshape(-1)
        n = rows.numel()
        return index, queries, count, ld, rows, n, device, excluded

    def similarity_ranks_device(self, queries, rows, thresholds, marks=None, *, exclude=None, workspace=None):
        '''Where a mark stands among ALL candidates of every query, left on the GPU, without the (Q, n) matrix of
        similarity_matrix_device in device memory: an int64 (Q,) tensor, counts[q] the number of candidates of row q of
        that matrix that PRECEDE the mark (thresholds[q], marks[q]) in similarity_topk_device's order -- a candidate at
        position c (an index into `rows`) with cosine v precedes it where v is greater than thresholds[q] (NaN above every
        number, -0.0 equal to +0.0), or equal and c < marks[q] (include/memb_hip_ranks.h). marks[q] = -1 counts the
        strictly greater cosines, the largest int64 the greater-or-equal ones; with marks[q] the position of a candidate
        and thresholds[q] the matrix's bits there, counts[q] is that candidate's 0-based rank: the slot it takes in
        similarity_topk_device's output. No k, no limit of 64. For trained models whose dim is a multiple of 4 and at most
        512 the matrix kernel fills a slice of the candidates in a workspace (about 32 MiB, independent of n) and two
        kernels (rank_count, rank_fold) count it; otherwise slices of at most 2^19 candidates go through
        similarity_matrix_device into one reused temporary and the same kernels (last_ranks_kernel says which).
        queries : as in similarity_matrix_device
        rows : as in similarity_topk_device; None: every row of the model in order, so positions are row ids
        thresholds : contiguous float32 (Q,) tensor on the same device
        marks : contiguous int64 (Q,) tensor on the same device; None: all -1
        exclude : as in similarity_topk_device: positions that are no candidates of their query and are not counted
        workspace : optional contiguous uint8 tensor on the same device, aligned to 8 bytes, of at least
            _memb_ranks.query_ranks_workspace_bytes(self._impl.context_handle(), Q, n, minimal=True) bytes, for the fused
            path: a call with it allocates nothing but its result (and the marks where None). Its size decides the
            slicing, never the result.
        One model, float32: the preceding candidates themselves are similarity_within_device's; no bfloat16 / float16, no
        ReadersUnion, no ShardedReader, no pooled-bag candidates, no ranks under the 3CosMul score.'''
        import torch
        index, queries, count, ld, rows, n, device, excluded = self._marks_arguments(torch, queries, rows, thresholds, marks, exclude)
        context = self._impl.context_handle()
        fused = _memb_ranks.query_ranks_kernel_name(context)
        if fused or n == 0:
            if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1
                                          or not workspace.is_contiguous() or workspace.device != device):
                raise TypeError('workspace must be a contiguous uint8 tensor on cuda:{}'.format(index))
        counts = torch.empty((count,), dtype=torch.int64, device=device)
        self._last_ranks_kernel = fused if count else ''
        if count == 0:   # (nothing is launched)
            return counts
        if marks is None:
            marks = torch.full((count,), -1, dtype=torch.int64, device=device)
        stream = _current_stream(torch, index)
        if fused or n == 0:
            if not fused:   # (no candidate: rank_fold alone writes the zeros, whatever the model)
                self._last_ranks_kernel = 'rank_fold'
            if workspace is None:
                workspace = torch.empty((_memb_ranks.query_ranks_workspace_bytes(context, count, n),), dtype=torch.uint8, device=device)
            done = _memb_ranks.query_ranks_to_device(
                context, queries.data_ptr(), count, ld, rows.data_ptr(), n, thresholds.data_ptr(), marks.data_ptr(), *excluded,
                counts.data_ptr(), workspace.data_ptr() if workspace.numel() else 0, workspace.numel(), stream)
            assert done   # (n == 0 is answered for every model)
            return counts
        width = min(n, QUERY_DEVICE_SLICE)
        temporary = torch.empty((count, width), dtype=torch.float32, device=device)
        partials = torch.empty((_memb_ranks.dense_ranks_workspace_bytes(count, width),), dtype=torch.uint8, device=device)
        for start in range(0, n, QUERY_DEVICE_SLICE):
            size = min(n, start + QUERY_DEVICE_SLICE) - start
            self.similarity_matrix_device(queries, rows[start:start + size], out=temporary[:, :size])
            _memb_ranks.dense_ranks_to_device(
                index, temporary.data_ptr(), count, size, width, start, thresholds.data_ptr(), marks.data_ptr(), *excluded,
                start > 0, counts.data_ptr(), partials.data_ptr(), partials.numel(), stream)
        self._last_ranks_kernel = self._last_query_matrix_kernel + '+' + _memb_ranks.dense_ranks_kernel_name()
        return counts

    def _host_marks_arguments(self, queries, rows, thresholds, marks, exclude):
        """the checks similarity_ranks and similarity_within share: (queries (Q, dim), Q, rows uint32, thresholds, marks,
        exclude int64 (Q, E) or None), contiguous"""
        queries = np.asarray(queries)
        if queries.dtype != np.float32:
            raise TypeError('queries must be a float32 array of shape (Q, dim) or (dim,)')
        if queries.ndim == 1:
            queries = queries[None, :]
        if queries.ndim != 2 or queries.shape[1] != self.dim:
            raise ValueError('queries must have shape (Q, {}) or ({},), got {}'.format(self.dim, self.dim, queries.shape))
        queries = np.ascontiguousarray(queries)
        count = queries.shape[0]
        thresholds, marks = rank_marks(thresholds, marks, count)
        rows = np.arange(len(self), dtype=np.uint32) if rows is None else np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
        if exclude is not None:
            exclude = np.asarray(exclude)
            if exclude.dtype.kind not in 'iu':
                raise TypeError('exclude must be an integer array of shape (Q, E)')
            if exclude.ndim != 2 or exclude.shape[0] != count:
                raise ValueError('exclude must have shape (Q, E) = ({}, E), got {}'.format(count, exclude.shape))
            if exclude.shape[1] > QUERY_TOPK_MAX_EXCLUDED:
                raise ValueError('exclude names at most {} positions per query, got {}'.format(QUERY_TOPK_MAX_EXCLUDED, exclude.shape[1]))
            exclude = np.ascontiguousarray(exclude, dtype=np.int64)
        return queries, count, rows, thresholds, marks, exclude

    def similarity_ranks(self, queries, rows, thresholds, marks=None, exclude=None):
        '''similarity_ranks_device for host arrays: a numpy float32 (Q, dim) or (dim,) array of queries, numpy row ids
        (None: every row of the model), float32 (Q,) thresholds and int64 (Q,) marks (None: all -1) in, a numpy int64 (Q,)
        array of counts out. A reader on a GPU sends everything up and brings the counts back; a device='cpu' reader takes
        similarity_matrix chunk by chunk and counts in numpy (ranks_host): the same numbers. exclude: an integer (Q, E)
        array, E <= 64.'''
        queries, count, rows, thresholds, marks, exclude = self._host_marks_arguments(queries, rows, thresholds, marks, exclude)
        if self._impl.device() != _memb.HOST_DEVICE:
            import torch
            device = 'cuda:{}'.format(self._impl.device())
            return self.similarity_ranks_device(
                torch.from_numpy(queries).to(device), torch.from_numpy(rows.view(np.int32)).to(device),
                torch.from_numpy(thresholds).to(device), torch.from_numpy(marks).to(device),
                exclude=None if exclude is None else torch.from_numpy(exclude).to(device)).cpu().numpy()
        counts = np.zeros(count, dtype=np.int64)
        for start in range(0, rows.size, NORMS_HOST_CHUNK):
            counts += ranks_host(self.similarity_matrix(queries, rows[start:start + NORMS_HOST_CHUNK]), thresholds, marks, start, exclude)
        return counts

    def rank_device(self, words_a, words_b):
        '''gensim's rank(a, b) for pairs of words, left on the GPU: an int64 (P,) tensor, for pair i one plus the number of
        words of the WHOLE model that precede words_b[i] around the unit row of words_a[i] -- 1 where words_b[i] is the
        nearest word of words_a[i], which is itself no candidate. The threshold is query_similarity_device of the unit row
        against the one row of words_b[i], bit for bit the entry of similarity_matrix_device there, the mark is that row,
        the rest is similarity_ranks_device over every row with words_a[i] as the one non-candidate: the 1-based slot
        words_b[i] takes in most_similar_device(words_a[i]) however far down that is. 0 where either word is not in the
        model.'''
        import torch
        index = self._impl.device()
        if index == _memb.HOST_DEVICE:
            raise RuntimeError("this reader decodes on the host (device 'cpu'): device buffers need a reader on a HIP device")
        words_a, words_b = list(words_a), list(words_b)
        if len(words_a) != len(words_b):
            raise ValueError('words_a and words_b must hold one word per pair, got {} and {}'.format(len(words_a), len(words_b)))
        device = 'cuda:{}'.format(index)
        count = len(words_a)
        if count == 0:
            return torch.empty((0,), dtype=torch.int64, device=device)
        own = self.resolve_rows_device(words_a + words_b)
        first, second = own[:count].contiguous(), own[count:].contiguous()
        queries = self.unit_rows_embedding_device(first)
        return self._ranks_of_marks(torch, queries, second, first.to(torch.int64).unsqueeze(1), (first < 0) | (second < 0))

    def _ranks_of_marks(self, torch, queries, expected, exclude, unanswered):
        """the 1-based rank of the row expected[q] (int32, -1: not in the model) around queries[q] over the whole model
        without the positions exclude[q]; 0 where unanswered[q]"""
        count = queries.shape[0]
        groups = torch.arange(count + 1, dtype=torch.int32, device=queries.device)
        thresholds = self.query_similarity_device(queries, expected, groups)   # (one candidate per group: the matrix's bits)
        counts = self.similarity_ranks_device(queries, None, thresholds, expected.to(torch.int64), exclude=exclude)
        return torch.where(unanswered, torch.zeros_like(counts), counts + 1)

    def rank(self, words_a, words_b):
        '''rank_device on the host: a numpy int64 (P,) array of 1-based ranks, 0 where a word is not in the model. A
        device='cpu' reader goes through unit_rows_embedding, query_similarity and similarity_ranks: the same numbers.'''
        words_a, words_b = list(words_a), list(words_b)
        if len(words_a) != len(words_b):
            raise ValueError('words_a and words_b must hold one word per pair, got {} and {}'.format(len(words_a), len(words_b)))
        count = len(words_a)
        if count == 0:
            return np.zeros(0, dtype=np.int64)
        if self._impl.device() != _memb.HOST_DEVICE:
            return self.rank_device(words_a, words_b).cpu().numpy()
        own = self.resolve_rows(words_a + words_b)
        first, second = own[:count], own[count:]
        missing = (first == 0xFFFFFFFF) | (second == 0xFFFFFFFF)
        exclude = np.where(first == 0xFFFFFFFF, -1, first.astype(np.int64))[:, None]
        return self._ranks_of_marks_host(self.unit_rows_embedding(first), second, exclude, missing)

    def _ranks_of_marks_host(self, queries, expected, exclude, unanswered):
        """_ranks_of_marks of a device='cpu' reader: expected uint32 rows (0xFFFFFFFF: not in the model)"""
        count = queries.shape[0]
        thresholds = self.query_similarity(queries, expected, np.arange(count + 1))
        marks = np.where(expected == 0xFFFFFFFF, -1, expected.astype(np.int64))
        counts = self.similarity_ranks(queries, None, thresholds, marks, exclude=exclude)
        return np.where(unanswered, 0, counts + 1)

    def count_closer_than(self, words_a, words_b):
        '''len(gensim's closer_than(a, b)) for pairs of words: a numpy int64 (P,) array, the number of words of the whole
        model closer to words_a[i] than words_b[i] is (words_a[i] itself left out; equal cosines: the lower row first) --
        rank(words_a, words_b) - 1, so -1 where a word is not in the model.'''
        return self.rank(words_a, words_b) - 1

    def analogy_ranks_device(self, positive, negative, expected):
        '''The rank of the EXPECTED answer of every analogy question, left on the GPU: an int64 (Q,) tensor, 1 where
        analogies_device(positive, negative, k=1) answers expected[q], 2 where it is the second best word, and so on down
        the whole vocabulary -- what mean reciprocal rank and hits@k for any k are made of. The queries are
        analogies_device's composed queries, a question's own words are no candidates, the mark is the row of expected[q]
        with its cosine against the query as the threshold (query_similarity_device: the matrix's bits). 0 where a word
        of the question or the expected word is not in the model, or the question has no word.
        positive, negative : as in analogies_device (negative may be None)
        expected : one word per question'''
        import torch
        index = self._impl.device()
        if index == _memb.HOST_DEVICE:
            raise RuntimeError("this reader decodes on the host (device 'cpu'): device buffers need a reader on a HIP device")
        device = 'cuda:{}'.format(index)
        words, weights, offsets, members = self._analogy_entries(positive, negative)
        expected = list(expected)
        count = offsets.size - 1
        if len(expected) != count:
            raise ValueError('expected must hold one word per question, got {} for {}'.format(len(expected), count))
        if count == 0:
            return torch.empty((0,), dtype=torch.int64, device=device)
        own = self.resolve_rows_device(words + expected)
        answers = own[len(words):].contiguous()
        own = own[:len(words)].contiguous()
        queries = self.compose_queries_device(
            own, torch.from_numpy(offsets.astype(np.int32)).to(device), torch.from_numpy(weights).to(device))
        members = torch.from_numpy(members).to(device)
        padded = torch.cat([own.to(torch.int64), torch.full((1,), -1, dtype=torch.int64, device=device)])   # (a missing word is -1)
        exclude = padded[members]   # (members == -1 reads the -1 at the end)
        unanswered = ((members >= 0) & (exclude < 0)).any(dim=1) | torch.from_numpy(offsets[1:] == offsets[:-1]).to(device) | (answers < 0)
        return self._ranks_of_marks(torch, queries, answers, exclude, unanswered)

    def analogy_ranks(self, positive, negative, expected):
        '''analogy_ranks_device on the host: a numpy int64 (Q,) array of 1-based ranks, 0 where a question is not
        answered. A device='cpu' reader goes through compose_queries, query_similarity and similarity_ranks: the same
        numbers.'''
        if self._impl.device() != _memb.HOST_DEVICE:
            return self.analogy_ranks_device(positive, negative, expected).cpu().numpy()
        words, weights, offsets, members = self._analogy_entries(positive, negative)
        expected = list(expected)
        count = offsets.size - 1
        if len(expected) != count:
            raise ValueError('expected must hold one word per question, got {} for {}'.format(len(expected), count))
        if count == 0:
            return np.zeros(0, dtype=np.int64)
        own = self.resolve_rows(words + expected)
        answers, own = own[len(words):], own[:len(words)]
        rows = np.concatenate([np.where(own == 0xFFFFFFFF, -1, own.astype(np.int64)), [-1]])
        exclude = rows[members]
        unanswered = ((members >= 0) & (exclude < 0)).any(axis=1) | (offsets[1:] == offsets[:-1]) | (answers == 0xFFFFFFFF)
        return self._ranks_of_marks_host(self.compose_queries(own, offsets, weights), answers, exclude, unanswered)

    def evaluate_analogies(self, questions):
        '''An analogy test set in one pass: questions is an iterable of (a, b, c, expected) -- a is to b as c is to
        expected, as the lines of the Google analogy set. Returns a dict: 'questions' (how many were given), 'answered'
        (those whose four words the model knows; the others count nowhere else, as in gensim's evaluation), 'accuracy'
        (the share of the answered ones whose expected word is the best candidate, a, b and c left out: rank 1) and
        'mean_reciprocal_rank' (the mean of 1 / rank over the answered ones), both 0.0 where none is answered. The ranks
        are analogy_ranks([[b, c]], [[a]], [expected]) for all questions at once; the figures are worked out on the host.'''
        questions = [tuple(question) for question in questions]
        for question in questions:
            if len(question) != 4:
                raise ValueError('a question is (a, b, c, expected), got {!r}'.format(question))
        ranks = self.analogy_ranks([[b, c] for _, b, c, _ in questions], [[a] for a, _, _, _ in questions],
                                   [expected for _, _, _, expected in questions])
        answered = ranks[ranks > 0]
        return {
            'questions': len(questions),
            'answered': int(answered.size),
            'accuracy': float((answered == 1).sum() / answered.size) if answered.size else 0.0,
            'mean_reciprocal_rank': float((1.0 / answered).mean()) if answered.size else 0.0,
        }

    # ---- the candidates that precede a mark, listed: closer_than as words, a radius search (include/memb_hip_within.h) ----

    @property
    def last_within_kernel(self):
        '''The kernel families of the last fill of similarity_within_device, joined by '+':
        'query_matrix_trained+within_count+within_starts+within_write' (slices of the fused matrix kernel in a workspace,
        compacted there), or 'pairs_dense+within_count+within_starts+within_write' where the cosines of a slice come from
        similarity_matrix_device's fallback -- uniform and full storage, dims that are no multiple of 4 or beyond 512;
        'within_starts' where such a model is asked with no candidate at all. '' before any call and after a call without
        queries, which launches nothing. Informational: the lists are the same.'''
        return self._last_within_kernel

    def similarity_within_device(self, queries, rows, thresholds, marks=None, *, exclude=None, return_values=True, offsets=None,
                                 capacity=None, workspace=None):
        '''The candidates similarity_ranks_device COUNTS, themselves, left on the GPU, without the (Q, n) matrix of
        similarity_matrix_device in device memory: (offsets, positions, values) in CSR form -- offsets an int64 (Q + 1,)
        tensor, positions an int64 (total,) tensor and values a float32 (total,) tensor (None with return_values=False).
        positions[offsets[q]:offsets[q + 1]] are the candidates of query q (indices into `rows`) that precede the mark
        (thresholds[q], marks[q]) and are not named by exclude[q], ASCENDING, and values holds the matrix's bits there
        (include/memb_hip_within.h). marks[q] = -1 lists the cosines strictly greater than thresholds[q], the largest int64
        the greater-or-equal ones: every candidate within a radius, however many. The result depends on the arguments
        alone, never on the slicing. For trained models whose dim is a multiple of 4 and at most 512 the matrix kernel fills
        a slice of the candidates in a workspace and three kernels (within_count, within_starts, within_write) compact it
        in order; otherwise slices of at most 2^19 candidates go through similarity_matrix_device into one reused temporary
        and the same kernels (last_within_kernel says which).
        queries, rows, thresholds, marks, exclude : as in similarity_ranks_device
        offsets : None: the sizes come from similarity_ranks_device -- a second pass over the candidates --, their running
            sum is the offsets and its last entry is read on the host to size the result: ONE synchronisation. Or a
            contiguous int64 (Q + 1,) tensor on the same device, non-decreasing from offsets[0] >= 0: the segments the
            caller chose, filled by the one call, and the result is (offsets, positions, values, found), found an int64
            (Q,) tensor of what each query found whatever its segment holds. A segment that is too short keeps the first
            entries of its list and found[q] > offsets[q + 1] - offsets[q] says so; nothing is written outside it.
        capacity : with offsets given, the entries positions and values are allocated with (what lies outside every
            segment is left as allocated); the call then synchronises nothing and can be captured into a graph. None:
            offsets[Q] is read on the host, one synchronisation. Nothing checks that capacity covers offsets[Q]: entries
            whose place lies at or beyond capacity are dropped like those beyond a segment's end, and only
            found[q] > min(offsets[q + 1], capacity) - offsets[q] tells.
        workspace : optional contiguous uint8 tensor on the same device, aligned to 8 bytes, of at least
            _memb_within.query_within_workspace_bytes(self._impl.context_handle(), Q, n, minimal=True) bytes, for the fused
            path (it serves the count pass too). Its size decides the slicing, never the result.
        One model, float32: no bfloat16 / float16, no ReadersUnion, no ShardedReader, no pooled-bag candidates, no lists
        under the 3CosMul score, no output sorted by cosine (torch.sort of a segment of values does that).'''
        import torch
        index, queries, count, ld, rows, n, device, excluded = self._marks_arguments(torch, queries, rows, thresholds, marks, exclude)
        context = self._impl.context_handle()
        fused = _memb_within.query_within_kernel_name(context)
        if workspace is not None and (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1
                                      or not workspace.is_contiguous() or workspace.device != device):
            raise TypeError('workspace must be a contiguous uint8 tensor on cuda:{}'.format(index))
        given = offsets is not None
        if given:
            if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int64:
                raise TypeError('offsets must be an int64 tensor of shape (Q + 1,)')
            if offsets.device != device:
                raise ValueError('offsets must be on {} (the device this reader is staged on), got {}'.format(device, offsets.device))
            if offsets.dim() != 1 or offsets.shape[0] != count + 1 or not offsets.is_contiguous():
                raise ValueError('offsets must be contiguous with shape (Q + 1,) = ({},), got {}'.format(count + 1, tuple(offsets.shape)))
            if capacity is not None and (isinstance(capacity, bool) or int(capacity) != capacity or capacity < 0):
                raise ValueError('capacity must be a non-negative integer, got {!r}'.format(capacity))
        elif capacity is not None:
            raise ValueError('capacity goes with offsets: without them the call sizes its result itself')
        self._last_within_kernel = ''
        if not given:
            counts = self.similarity_ranks_device(queries, rows, thresholds, marks, exclude=exclude, workspace=workspace)
            offsets = torch.zeros((count + 1,), dtype=torch.int64, device=device)
            torch.cumsum(counts, 0, out=offsets[1:])
        if capacity is None:
            capacity = offsets[-1].item()   # (the one synchronisation)
        capacity = int(capacity)
        # (at least one entry is allocated, so that the outputs have an address where nothing is to be listed)
        held_positions = torch.empty((max(capacity, 1),), dtype=torch.int64, device=device)
        held_values = torch.empty((max(capacity, 1),), dtype=torch.float32, device=device) if return_values else None
        positions, values = held_positions[:capacity], held_values[:capacity] if return_values else None
        found = torch.empty((count,), dtype=torch.int64, device=device)
        result = (offsets, positions, values, found) if given else (offsets, positions, values)
        if count == 0:   # (nothing is launched)
            return result
        if marks is None:
            marks = torch.full((count,), -1, dtype=torch.int64, device=device)
        stream = _current_stream(torch, index)
        output = (offsets.data_ptr(), found.data_ptr(), held_positions.data_ptr(), held_values.data_ptr() if return_values else 0, capacity)
        if fused or n == 0:
            self._last_within_kernel = fused or 'within_starts'   # (no candidate: within_starts alone writes zeros, whatever the model)
            if workspace is None:
                workspace = torch.empty((_memb_within.query_within_workspace_bytes(context, count, n),), dtype=torch.uint8, device=device)
            done = _memb_within.query_within_to_device(
                context, queries.data_ptr(), count, ld, rows.data_ptr(), n, thresholds.data_ptr(), marks.data_ptr(), *excluded,
                *output, workspace.data_ptr() if workspace.numel() else 0, workspace.numel(), stream)
            assert done   # (n == 0 is answered for every model)
            return result
        width = min(n, QUERY_DEVICE_SLICE)
        temporary = torch.empty((count, width), dtype=torch.float32, device=device)
        blocks = torch.empty((_memb_within.dense_within_workspace_bytes(count, width),), dtype=torch.uint8, device=device)
        for start in range(0, n, QUERY_DEVICE_SLICE):   # (ascending, as the lists are)
            size = min(n, start + QUERY_DEVICE_SLICE) - start
            self.similarity_matrix_device(queries, rows[start:start + size], out=temporary[:, :size])
            _memb_within.dense_within_to_device(
                index, temporary.data_ptr(), count, size, width, start, thresholds.data_ptr(), marks.data_ptr(), *excluded,
                start > 0, *output, blocks.data_ptr(), blocks.numel(), stream)
        self._last_within_kernel = self._last_query_matrix_kernel + '+' + _memb_within.dense_within_kernel_name()
        return result

    def similarity_within(self, queries, rows, thresholds, marks=None, exclude=None):
        '''similarity_within_device for host arrays: numpy queries, row ids (None: every row of the model), float32 (Q,)
        thresholds and int64 (Q,) marks (None: all -1) in, numpy (offsets int64 (Q + 1,), positions int64 (total,), values
        float32 (total,)) out. A reader on a GPU sends everything up and brings the lists back; a device='cpu' reader takes
        similarity_matrix chunk by chunk and lists in numpy (within_host): the same bits. exclude: an integer (Q, E) array,
        E <= 64.'''
        queries, count, rows, thresholds, marks, exclude = self._host_marks_arguments(queries, rows, thresholds, marks, exclude)
        if self._impl.device() != _memb.HOST_DEVICE:
            import torch
            device = 'cuda:{}'.format(self._impl.device())
            return tuple(part.cpu().numpy() for part in self.similarity_within_device(
                torch.from_numpy(queries).to(device), torch.from_numpy(rows.view(np.int32)).to(device),
                torch.from_numpy(thresholds).to(device), torch.from_numpy(marks).to(device),
                exclude=None if exclude is None else torch.from_numpy(exclude).to(device)))
        chunks = [within_host(self.similarity_matrix(queries, rows[start:start + NORMS_HOST_CHUNK]), thresholds, marks, start, exclude)
                  for start in range(0, rows.size, NORMS_HOST_CHUNK)]
        offsets = np.zeros(count + 1, dtype=np.int64)
        np.cumsum(sum((np.diff(chunk[0]) for chunk in chunks), np.zeros(count, dtype=np.int64)), out=offsets[1:])
        positions = np.empty(offsets[-1], dtype=np.int64)
        values = np.empty(offsets[-1], dtype=np.float32)
        filled = offsets[:-1].copy()   # (where row q goes on: the chunks come in ascending order)
        for chunk_offsets, chunk_positions, chunk_values in chunks:
            sizes = np.diff(chunk_offsets)
            of_row = np.repeat(np.arange(count), sizes)
            target = filled[of_row] + np.arange(chunk_positions.size) - chunk_offsets[of_row]
            positions[target], values[target] = chunk_positions, chunk_values
            filled += sizes
        return offsets, positions, values

    @staticmethod
    def _no_list_where(torch, unanswered, thresholds, marks):
        """the marks of queries that list nothing: a NaN threshold has the greatest key, and no position is below -1"""
        return (torch.where(unanswered, torch.full_like(thresholds, float('nan')), thresholds),
                torch.where(unanswered, torch.full_like(marks, -1), marks))

    def closer_than_device(self, words_a, words_b):
        '''gensim's closer_than(a, b) for pairs of words, left on the GPU: (offsets, rows), an int64 (P + 1,) and an int64
        (total,) tensor -- rows[offsets[i]:offsets[i + 1]] are the row ids (positions in keys()), ascending, of the words of
        the WHOLE model that are closer to words_a[i] than words_b[i] is: exactly the words rank_device counts, so
        offsets[i + 1] - offsets[i] == rank_device(...)[i] - 1. words_a[i] itself is no candidate; equal cosines: the lower
        row is the closer one. An empty list where either word is not in the model. One synchronisation
        (similarity_within_device's).'''
        import torch
        index = self._impl.device()
        if index == _memb.HOST_DEVICE:
            raise RuntimeError("this reader decodes on the host (device 'cpu'): device buffers need a reader on a HIP device")
        words_a, words_b = list(words_a), list(words_b)
        if len(words_a) != len(words_b):
            raise ValueError('words_a and words_b must hold one word per pair, got {} and {}'.format(len(words_a), len(words_b)))
        device = 'cuda:{}'.format(index)
        count = len(words_a)
        if count == 0:
            return torch.zeros((1,), dtype=torch.int64, device=device), torch.empty((0,), dtype=torch.int64, device=device)
        own = self.resolve_rows_device(words_a + words_b)
        first, second = own[:count].contiguous(), own[count:].contiguous()
        queries = self.unit_rows_embedding_device(first)
        groups = torch.arange(count + 1, dtype=torch.int32, device=queries.device)
        thresholds = self.query_similarity_device(queries, second, groups)   # (one candidate per group: the matrix's bits)
        thresholds, marks = self._no_list_where(torch, (first < 0) | (second < 0), thresholds, second.to(torch.int64))
        offsets, rows, _ = self.similarity_within_device(
            queries, None, thresholds, marks, exclude=first.to(torch.int64).unsqueeze(1), return_values=False)
        return offsets, rows

    def closer_than(self, a, b):
        '''gensim's closer_than(a, b): the list of the words of the whole model that are closer to the word a than the word
        b is, in row order (the order of keys()); a itself is no candidate, equal cosines: the lower row is the closer one.
        len() of it is count_closer_than([a], [b])[0]. [] where a or b is not in the model. closer_than_device on a GPU
        reader; a device='cpu' reader goes through unit_rows_embedding, query_similarity and similarity_within: the same
        words.'''
        if self._impl.device() != _memb.HOST_DEVICE:
            rows = self.closer_than_device([a], [b])[1].cpu().numpy()
        else:
            own = self.resolve_rows([a, b])
            if (own == 0xFFFFFFFF).any():
                return []
            queries = self.unit_rows_embedding(own[:1])
            thresholds = self.query_similarity(queries, own[1:], np.arange(2))
            rows = self.similarity_within(queries, None, thresholds, own[1:].astype(np.int64), exclude=own[:1].astype(np.int64)[:, None])[1]
        vocabulary = self.keys()
        return [vocabulary[row] for row in rows]

    @staticmethod
    def _min_cosine(min_cosine):
        """min_cosine as a float32; TypeError / ValueError unless it is a number"""
        if isinstance(min_cosine, bool) or not isinstance(min_cosine, numbers.Real):
            raise TypeError('min_cosine must be a number')
        if np.isnan(min_cosine):
            raise ValueError('min_cosine must be a number, got NaN')
        return np.float32(min_cosine)

    def words_within_device(self, words, min_cosine):
        '''Every word within a radius of each word, left on the GPU: (offsets, rows, values), an int64 (len(words) + 1,), an
        int64 (total,) and a float32 (total,) tensor -- rows[offsets[i]:offsets[i + 1]] are the row ids, ascending, of the
        words of the WHOLE model whose cosine to words[i] is at least min_cosine (compared as float32), the word itself
        left out, and values their cosines: similarity_within_device with the mark at the largest int64. An empty list for
        a word that is not in the model. One synchronisation.'''
        import torch
        index = self._impl.device()
        if index == _memb.HOST_DEVICE:
            raise RuntimeError("this reader decodes on the host (device 'cpu'): device buffers need a reader on a HIP device")
        min_cosine = self._min_cosine(min_cosine)
        words = list(words)
        device = 'cuda:{}'.format(index)
        if not words:
            return (torch.zeros((1,), dtype=torch.int64, device=device), torch.empty((0,), dtype=torch.int64, device=device),
                    torch.empty((0,), dtype=torch.float32, device=device))
        own = self.resolve_rows_device(words)
        thresholds = torch.full((len(words),), float(min_cosine), dtype=torch.float32, device=device)
        marks = torch.full((len(words),), np.iinfo(np.int64).max, dtype=torch.int64, device=device)
        thresholds, marks = self._no_list_where(torch, own < 0, thresholds, marks)
        return self.similarity_within_device(self.unit_rows_embedding_device(own), None, thresholds, marks, exclude=own.to(torch.int64).unsqueeze(1))

    def words_within(self, words, min_cosine):
        '''Every word within a radius of each word, on the host: one list of (word, cosine) pairs per word, in row order
        (the order of keys()), with cosine >= min_cosine, the word itself left out; [] for a word the model lacks.
        words_within_device on a GPU reader, similarity_within on a device='cpu' reader: the same pairs.'''
        min_cosine = self._min_cosine(min_cosine)
        words = list(words)
        if not words:
            return []
        if self._impl.device() != _memb.HOST_DEVICE:
            offsets, rows, values = (part.cpu().numpy() for part in self.words_within_device(words, min_cosine))
        else:
            own = self.resolve_rows(words)
            missing = own == 0xFFFFFFFF
            thresholds = np.where(missing, np.float32(np.nan), min_cosine).astype(np.float32)
            marks = np.where(missing, -1, np.iinfo(np.int64).max).astype(np.int64)
            exclude = np.where(missing, -1, own.astype(np.int64))[:, None]
            offsets, rows, values = self.similarity_within(self.unit_rows_embedding(own), None, thresholds, marks, exclude=exclude)
        vocabulary = self.keys()
        return [[(vocabulary[row], float(value)) for row, value in zip(rows[offsets[i]:offsets[i + 1]], values[offsets[i]:offsets[i + 1]])]
                for i in range(len(words))]

    # ---- every query against every pooled bag of rows, matrix and top-k (include/memb_hip_query_bags.h) ----

    @property
    def last_query_bags_kernel(self):
        '''The kernel family of the last bag_similarity_matrix_device call: 'query_bags_trained' (fused with the pooling) or
        'pairs_dense' behind a pooled lookup of a slice of the bags -- uniform and full storage, dims that are no multiple
        of 4 or beyond 512. '' before any call. Informational: the bits are the same.'''
        return self._last_query_bags_kernel

    @property
    def last_query_bags_topk_kernel(self):
        '''The kernel families of the last bag_similarity_topk_device call, joined by '+':
        'query_bags_trained+topk_select+topk_merge' (slices of the fused kernel in a workspace, selected there), or
        'pairs_dense+topk_select+topk_merge' where the matrix of a slice comes from bag_similarity_matrix_device's fallback;
        'topk_merge' where such a model is asked with no bag at all. '' before any call and after a call without queries,
        which launches nothing. Informational: the bits are the same.'''
        return self._last_query_bags_topk_kernel

    def _bag_arguments(self, torch, rows, offsets, index, device):
        '''bags_embedding_device's checks on its offsets; returns the number of bags'''
        if (not isinstance(offsets, torch.Tensor) or offsets.device.type != 'cuda' or offsets.dtype not in (torch.int32, torch.uint32)
                or not offsets.is_contiguous() or offsets.dim() != 1):
            raise TypeError('offsets must be a contiguous int32/uint32 tensor of bags + 1 entries on the GPU')
        if offsets.numel() < 1:
            raise ValueError('offsets needs bags + 1 entries')
        if device.index != index or offsets.device != device:
            raise ValueError('rows and offsets must be on cuda:{} (the device this reader is staged on), got {} and {}'.format(
                self.device, device, offsets.device))
        return offsets.numel() - 1

    @staticmethod
    def _bag_slice(torch, flat, offsets, start, stop):
        '''(entries, offsets) of the bags [start, stop) for a pooled launch of their own: the slice's offsets as the kernel
        clamps them, rebased on the slice's lowest entry so that the launch is planned for the slice's entries alone --
        made on the device, with one scalar read back to cut those entries out of `rows`. All bags: as they are.'''
        if start == 0 and stop == offsets.numel() - 1:
            return flat, offsets
        cut = offsets[start:stop + 1].view(torch.int32).to(torch.int64) & 0xFFFFFFFF
        cut = torch.clamp(cut, max=flat.numel())
        first = int(cut.min())
        return flat[first:], (cut - first).to(torch.int32)

    def _bag_matrix_fallback(self, torch, queries, count, flat, offsets, start, stop, mode, temporary, out, dots, norms, stream):
        '''the bags [start, stop) pooled ONCE into temporary[:, 1], then every query written beside the same pooled rows and
        reduced by the dense pair kernel into out[:, :stop - start] (dots likewise; norms: the pooled rows')'''
        index, dim, size = self._impl.device(), self.dim, stop - start
        entries, cut = self._bag_slice(torch, flat, offsets, start, stop)
        self.bags_embedding_device(entries, cut, mode=mode, out=temporary.view(temporary.shape[0], 2 * dim)[:size], col_off=dim)
        pair_norms = torch.empty((size, 2), dtype=torch.float32, device=flat.device) if norms is not None else None
        for q in range(count):
            temporary[:size, 0] = queries[q]
            _memb.dense_pair_similarity_to_device(
                index, temporary.data_ptr(), size, dim, dim, out[q, :size].data_ptr() if out is not None else 0,
                dots[q, :size].data_ptr() if dots is not None else 0,
                pair_norms.data_ptr() if norms is not None and q == 0 else 0, stream)
            if norms is not None and q == 0:
                norms[:size] = pair_norms[:, 1]

    def bag_similarity_matrix_device(self, queries, rows, offsets, mode='mean', *, return_dots=False, return_norms=False, out=None):
        '''The cosine similarity of EVERY query vector against EVERY pooled bag of rows, left on the GPU: a float32 (Q, bags)
        tensor, cos[q, b] of query q and the sum or mean of bag b -- query vectors against a corpus of sentences as
        averaged word vectors. For trained models whose dim is a multiple of 4 and at most 512 ONE kernel pools every bag in
        registers, scores it against all queries and writes neither a pooled nor a decoded row; otherwise slices of at most
        2^16 bags are pooled once into a reused temporary (bags_embedding_device) and reduced there against one query
        after the other (last_query_bags_kernel says which). Bit for bit the contract of include/memb_hip_query_bags.h:
        similarity_matrix_device's reduction with the rows bags_embedding_device(rows, offsets, mode) gives for its
        candidates -- whichever kernel ran. Not clamped. An empty bag, or a bag of rows that are not in the model, has cosine 0.
        queries : as in similarity_matrix_device (callers with sentences for queries pool them first:
            sentences_embedding_device)
        rows, offsets : as in bags_embedding_device, offsets holding bags + 1 entries
        mode : 'mean' or 'sum'
        return_dots, return_norms : either one returns (cosines, dots, norms) instead, dots a float32 (Q, bags) tensor and
            norms the pair (query_norms (Q,), bag_norms (bags,)) -- row_norms of the pooled rows --, None where not asked for
        out : optional float32 (Q, bags) tensor on the same device for the cosines, with a contiguous last dimension and a
            row stride of at least bags; nothing between its rows is written
        One model, float32, missing='zero', the sequential order: no missing='skip', no reduction='chunked', no bfloat16 /
        float16, no ReadersUnion, no ShardedReader.'''
        import torch
        code = pool_mode(mode)
        index, device = self._norms_arguments(torch, rows)
        dim = self.dim
        queries, count, ld = self._topk_queries(torch, queries, index)
        bags = self._bag_arguments(torch, rows, offsets, index, device)
        if out is None:
            out = torch.empty((count, bags), dtype=torch.float32, device=device)
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.dim() != 2 or tuple(out.shape) != (count, bags):
            raise TypeError('out must be a float32 (Q, bags) tensor')
        if (bags > 1 and out.stride(1) != 1) or (count > 1 and out.stride(0) < bags):
            raise ValueError('out must have a contiguous last dimension and a row stride of at least bags')
        if out.device != device or queries.device != device:
            raise ValueError('queries, rows and out must be on cuda:{} (the device this reader is staged on), got {}, {} and {}'.format(
                self.device, queries.device, device, out.device))
        ld_out = out.stride(0) if count > 1 else bags
        dots = torch.empty((count, bags), dtype=torch.float32, device=device) if return_dots else None
        bag_norms = torch.empty((bags,), dtype=torch.float32, device=device) if return_norms else None
        stream = _current_stream(torch, index)
        norms = None
        if return_norms:
            query_norms = torch.empty((count,), dtype=torch.float32, device=device)
            if count:
                _memb.dense_row_norms_to_device(index, queries.data_ptr(), count, dim, ld, query_norms.data_ptr(), stream)
            norms = (query_norms, bag_norms)
        result = (out, dots, norms) if return_dots or return_norms else out
        flat = rows.reshape(-1)
        self._last_query_bags_kernel = self._impl.query_bags_kernel_name() or _memb.dense_pairs_kernel_name()
        if bags == 0:
            return result
        if count == 0:   # (no query: the pooled rows' norms are all there is to work out)
            if return_norms:
                for start in range(0, bags, QUERY_BAGS_DEVICE_SLICE):
                    stop = min(bags, start + QUERY_BAGS_DEVICE_SLICE)
                    entries, cut = self._bag_slice(torch, flat, offsets, start, stop)
                    pooled = self.bags_embedding_device(entries, cut, mode=mode)
                    _memb.dense_row_norms_to_device(index, pooled.data_ptr(), stop - start, dim, dim, bag_norms[start:stop].data_ptr(), stream)
            return result
        if self._impl.query_bags_to_device(
                queries.data_ptr(), count, ld, flat.data_ptr(), flat.numel(), offsets.data_ptr(), bags, code, out.data_ptr(),
                dots.data_ptr() if return_dots else 0, ld_out, bag_norms.data_ptr() if return_norms else 0, stream):
            return result
        self._last_query_bags_kernel = _memb.dense_pairs_kernel_name()
        temporary = torch.empty((min(bags, QUERY_BAGS_DEVICE_SLICE), 2, dim), dtype=torch.float32, device=device)   # (query, pooled row) side by side
        for start in range(0, bags, QUERY_BAGS_DEVICE_SLICE):
            stop = min(bags, start + QUERY_BAGS_DEVICE_SLICE)
            self._bag_matrix_fallback(
                torch, queries, count, flat, offsets, start, stop, mode, temporary, out[:, start:stop],
                dots[:, start:stop] if return_dots else None, bag_norms[start:stop] if return_norms else None, stream)
        return result

    def bag_similarity_topk_device(self, queries, rows, offsets, k, mode='mean', *, workspace=None):
        '''The k most similar pooled bags of EVERY query, left on the GPU, without the (bags, dim) matrix of pooled rows and
        without the (Q, bags) matrix of bag_similarity_matrix_device in device memory: (values, positions), a float32 (Q, k)
        and an int64 (Q, k) tensor. Row q of bag_similarity_matrix_device(queries, rows, offsets, mode) in
        similarity_topk_device's order -- a stable descending sort, NaN first, equal cosines lower bag index first --, cut
        to k; positions are bag indices; where bags < k the last entries are empty: position -1, value -inf. One answer
        whatever the slicing. For trained models whose dim is a multiple of 4 and at most 512 the fused kernel fills a
        slice of the bags in a workspace (about 32 MiB, independent of the corpus) and the two selection kernels merge it
        into the result; otherwise slices of at most 2^16 bags go through bag_similarity_matrix_device's fallback into one
        reused temporary and the same selection (last_query_bags_topk_kernel says which).
        queries, rows, offsets, mode : as in bag_similarity_matrix_device
        k : 1 .. 64 (QUERY_TOPK_MAX_K)
        workspace : optional contiguous uint8 tensor on the same device, aligned to 8 bytes, of at least
            self._impl.query_bags_topk_workspace_bytes(Q, bags, k, minimal=True) bytes, for the fused path: a call with it
            allocates nothing but its two results. Its size decides the slicing, never the result.
        One model, float32: no k > 64, no missing='skip', no reduction='chunked', no bfloat16 / float16, no ReadersUnion, no
        ShardedReader.'''
        import torch
        code = pool_mode(mode)
        k = topk_size(k)
        index, device = self._norms_arguments(torch, rows)
        queries, count, ld = self._topk_queries(torch, queries, index)
        bags = self._bag_arguments(torch, rows, offsets, index, device)
        if queries.device != device:
            raise ValueError('queries and rows must be on cuda:{} (the device this reader is staged on), got {} and {}'.format(
                self.device, queries.device, device))
        flat = rows.reshape(-1)
        values = torch.empty((count, k), dtype=torch.float32, device=device)
        positions = torch.empty((count, k), dtype=torch.int64, device=device)
        stream = _current_stream(torch, index)
        fused = self._impl.query_bags_topk_kernel_name()
        self._last_query_bags_topk_kernel = fused if count else ''
        if count == 0:   # (nothing is launched)
            return values, positions
        if fused or bags == 0:
            if not fused:   # (no bag: topk_merge alone fills the empty slots, whatever the model)
                self._last_query_bags_topk_kernel = 'topk_merge'
            if workspace is None:
                workspace = torch.empty((self._impl.query_bags_topk_workspace_bytes(count, bags, k),), dtype=torch.uint8, device=device)
            elif (not isinstance(workspace, torch.Tensor) or workspace.dtype != torch.uint8 or workspace.dim() != 1
                    or not workspace.is_contiguous() or workspace.device != device):
                raise TypeError('workspace must be a contiguous uint8 tensor on cuda:{}'.format(index))
            done = self._impl.query_bags_topk_to_device(
                queries.data_ptr(), count, ld, flat.data_ptr(), flat.numel(), offsets.data_ptr(), bags, code, k,
                values.data_ptr(), positions.data_ptr(), k, workspace.data_ptr() if workspace.numel() else 0,
                workspace.numel(), stream)
            assert done   # (bags == 0 is answered for every model)
            return values, positions
        width = min(bags, QUERY_BAGS_DEVICE_SLICE)
        temporary = torch.empty((width, 2, self.dim), dtype=torch.float32, device=device)
        matrix = torch.empty((count, width), dtype=torch.float32, device=device)
        lists = torch.empty((topk_fallback_list_bytes(count, bags, k, QUERY_BAGS_DEVICE_SLICE),), dtype=torch.uint8, device=device)
        for start in range(0, bags, QUERY_BAGS_DEVICE_SLICE):
            stop = min(bags, start + QUERY_BAGS_DEVICE_SLICE)
            self._bag_matrix_fallback(torch, queries, count, flat, offsets, start, stop, mode, temporary, matrix, None, None, stream)
            _memb.dense_topk_to_device(
                index, matrix.data_ptr(), count, stop - start, width, start, k, start > 0, values.data_ptr(), positions.data_ptr(),
                k, lists.data_ptr(), lists.numel(), stream)
        self._last_query_bags_topk_kernel = _memb.dense_pairs_kernel_name() + '+' + _memb.dense_topk_kernel_name()
        return values, positions

    def nearest_sentences_device(self, query_sentences, corpus_sentences, k=10, mode='mean'):
        '''The k nearest sentences of a corpus for each query sentence, as pooled word vectors, left on the GPU: (values,
        positions), a float32 (len(query_sentences), k) tensor of cosines and an int64 tensor of indices into
        corpus_sentences, best first in similarity_topk_device's order. The queries are pooled by
        sentences_embedding_device(query_sentences, mode); the corpus is flattened (flatten_sentences), resolved on the
        device (resolve_rows_device) and never pooled into memory: the rest is bag_similarity_topk_device. An unknown word
        is a zero row that counts; a sentence without words has cosine 0. Slots beyond len(corpus_sentences) are position
        -1, value -inf.'''
        import torch
        pool_mode(mode)
        k = topk_size(k)
        index = self._impl.device()
        if index == _memb.HOST_DEVICE:
            raise RuntimeError("this reader decodes on the host (device 'cpu'): device buffers need a reader on a HIP device")
        device = 'cuda:{}'.format(index)
        queries = self.sentences_embedding_device(query_sentences, mode=mode)
        words, offsets = flatten_sentences(corpus_sentences)
        rows = self.resolve_rows_device(words) if words else torch.empty((0,), dtype=torch.int32, device=device)
        on_device = torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).to(device)
        return self.bag_similarity_topk_device(queries, rows, on_device, k, mode=mode)

    def _host_bag_arguments(self, queries, rows, offsets):
        queries = np.asarray(queries)
        if queries.dtype != np.float32:
            raise TypeError('queries must be a float32 array of shape (Q, dim) or (dim,)')
        if queries.ndim == 1:
            queries = queries[None, :]
        if queries.ndim != 2 or queries.shape[1] != self.dim:
            raise ValueError('queries must have shape (Q, {}) or ({},), got {}'.format(self.dim, self.dim, queries.shape))
        rows = np.ascontiguousarray(rows, dtype=np.uint32).reshape(-1)
        return np.ascontiguousarray(queries), rows, bag_offsets(offsets, rows.size)

    def _host_bag_slices(self, rows, offsets, mean):
        '''(start, stop, pooled rows of the bags [start, stop)) in slices of QUERY_BAGS_HOST_SLICE bags: bags_embedding's sums'''
        bags = offsets.size - 1
        for start in range(0, bags, QUERY_BAGS_HOST_SLICE):
            stop = min(bags, start + QUERY_BAGS_HOST_SLICE)
            cut = offsets[start:stop + 1]
            first, last = int(cut[0]), int(cut[-1])
            entries = rows[first:last]

            def slice_values(begin, end):
                yield self.rows_embedding(entries[begin:end])

            pooled, _ = pool_slices_host(cut - first, last - first, self.dim, BAGS_HOST_CHUNK, mean, False, slice_values)
            yield start, stop, pooled

    def bag_similarity_matrix(self, queries, rows, offsets, mode='mean', return_dots=False, return_norms=False):
        '''bag_similarity_matrix_device for host arrays: a numpy float32 (Q, dim) or (dim,) array of queries, numpy row ids
        and bags + 1 offsets (bags_embedding's: ascending, within 0 .. len(rows)) in, a numpy float32 (Q, bags) array of
        cosines out, or (cosines, dots, (query_norms, bag_norms)) with either flag (None where not asked for). A reader on
        a GPU sends everything up and brings the matrix back; a device='cpu' reader evaluates the same contract in numpy
        (pool_slices_host, pair_similarity_host) in bounded slices of bags, each pooled once for every query: the same bits.'''
        code = pool_mode(mode)
        queries, rows, offsets = self._host_bag_arguments(queries, rows, offsets)
        count, bags = queries.shape[0], offsets.size - 1
        if self._impl.device() != _memb.HOST_DEVICE:
            import torch
            device = 'cuda:{}'.format(self._impl.device())
            result = self.bag_similarity_matrix_device(
                torch.from_numpy(queries).to(device), torch.from_numpy(rows.view(np.int32)).to(device),
                torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).to(device), mode=mode, return_dots=return_dots,
                return_norms=return_norms)
            if not (return_dots or return_norms):
                return result.cpu().numpy()
            cosines, dots, norms = result
            return (cosines.cpu().numpy(), None if dots is None else dots.cpu().numpy(),
                    None if norms is None else tuple(part.cpu().numpy() for part in norms))
        cosines = np.zeros((count, bags), dtype=np.float32)
        dots = np.zeros((count, bags), dtype=np.float32)
        bag_norms = np.zeros(bags, dtype=np.float32)
        for start, stop, pooled in self._host_bag_slices(rows, offsets, code == _memb.POOL_MEAN):
            bag_norms[start:stop] = row_norms_host(pooled)
            for q in range(count):
                cosines[q, start:stop], dots[q, start:stop], _ = pair_similarity_host(np.broadcast_to(queries[q], pooled.shape), pooled)
        if return_dots or return_norms:
            return (cosines, dots if return_dots else None,
                    (row_norms_host(queries) if count else np.zeros(0, dtype=np.float32), bag_norms) if return_norms else None)
        return cosines

    def bag_similarity_topk(self, queries, rows, offsets, k, mode='mean'):
        '''bag_similarity_topk_device for host arrays: (values float32 (Q, k), positions int64 (Q, k)), positions being bag
        indices. A reader on a GPU sends everything up and brings the result back; a device='cpu' reader takes
        bag_similarity_matrix's slices one by one and selects by the same order in numpy (topk_host): the same bits.'''
        code = pool_mode(mode)
        queries, rows, offsets = self._host_bag_arguments(queries, rows, offsets)
        k = topk_size(k)
        count = queries.shape[0]
        if self._impl.device() != _memb.HOST_DEVICE:
            import torch
            device = 'cuda:{}'.format(self._impl.device())
            values, positions = self.bag_similarity_topk_device(
                torch.from_numpy(queries).to(device), torch.from_numpy(rows.view(np.int32)).to(device),
                torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).to(device), k, mode=mode)
            return values.cpu().numpy(), positions.cpu().numpy()
        values = np.full((count, k), -np.inf, dtype=np.float32)
        positions = np.full((count, k), -1, dtype=np.int64)
        for start, stop, pooled in self._host_bag_slices(rows, offsets, code == _memb.POOL_MEAN):
            matrix = np.zeros((count, stop - start), dtype=np.float32)
            for q in range(count):
                matrix[q] = pair_similarity_host(np.broadcast_to(queries[q], pooled.shape), pooled)[0]
            values, positions = topk_host(matrix, k, start, (values, positions))
        return values, positions

    def stage_words(self):
        '''Copy the model's keys to the GPU and build the hash table over them there (once; resolve_rows_device does it
        on first use). After this, info()['device_bytes'] includes the word index.'''
        self._impl.stage_words()

    def resolve_rows_device(self, words, out=None):
        '''resolve_rows on the GPU: the words are packed into pinned memory by pooled host threads, copied once, and
        looked up by one kernel in a hash table over the model's keys (the same answers as the host search -- the
        reference's lower_bound + strcmp, src/trained_compression.cpp:115-125 -- misses as 0xFFFFFFFF). Returns a
        torch.int32 tensor on this reader's device; nothing waits for the GPU, the row ids never visit the host.
        May be called from several threads at once (each call packs its words into a batch of its own).
        out : optional contiguous int32 / uint32 tensor of len(words) entries on this reader's device'''
        import torch
        index = self._impl.device()
        if index == _memb.HOST_DEVICE:
            raise RuntimeError("this reader decodes on the host (device 'cpu'): the device word search needs a reader on a HIP device")
        n = len(words)
        if out is None:
            out = torch.empty((n,), dtype=torch.int32, device='cuda:{}'.format(index))
        elif (out.device.type != 'cuda' or out.device.index != index or out.dtype not in (torch.int32, torch.uint32)
              or not out.is_contiguous() or out.numel() != n):
            raise TypeError('out must be a contiguous int32/uint32 tensor of len(words) entries on cuda:{}'.format(index))
        batch = self._word_batches.take(index)
        try:
            self._impl.words_to_rows_device(batch, words, out.data_ptr(), _current_stream(torch, index))
        finally:
            self._word_batches.give(batch)
        return out

    def resolve_packed_device(self, data, offsets, out=None):
        '''resolve_rows_device for words that are packed already (a tokenizer's output): word i is the UTF-8 bytes
        data[offsets[i]:offsets[i + 1]]. No str object is touched -- the walk over a list of 2.2 M str is a cache miss per
        word and the larger half of resolve_rows_device's time.
        data : bytes-like (bytes, bytearray, memoryview, numpy.uint8) with offsets n + 1 ascending integers (any integer
            array or sequence; a value outside 0 .. 0xFFFFFFFF is a ValueError, a non-integer dtype a TypeError) -- copied
            once into pinned memory by pooled threads (GIL released), the lookups of finished runs overlap the copy of later
            ones; or BOTH torch tensors on this reader's device (uint8, int32 / uint32): looked up in place
            (memb_hip_resolve_packed_device_bounded: a word whose offsets run backwards or reach past data.numel() is
            0xFFFFFFFF; int32 offsets are read as uint32).
        Returns the torch.int32 row ids on this reader's device (0xFFFFFFFF = not in the model).
        May be called from several threads at once (each call packs its words into a batch of its own).'''
        import torch
        index = self._impl.device()
        if index == _memb.HOST_DEVICE:
            raise RuntimeError("this reader decodes on the host (device 'cpu'): the device word search needs a reader on a HIP device")
        on_device = isinstance(data, torch.Tensor) or isinstance(offsets, torch.Tensor)
        n = int(offsets.numel() if isinstance(offsets, torch.Tensor) else len(offsets)) - 1
        if n < 0:
            raise ValueError('offsets needs n + 1 entries')
        if out is None:
            out = torch.empty((n,), dtype=torch.int32, device='cuda:{}'.format(index))
        elif (out.device.type != 'cuda' or out.device.index != index or out.dtype not in (torch.int32, torch.uint32)
              or not out.is_contiguous() or out.numel() != n):
            raise TypeError('out must be a contiguous int32/uint32 tensor of n entries on cuda:{}'.format(index))
        if on_device:
            if not (isinstance(data, torch.Tensor) and isinstance(offsets, torch.Tensor)):
                raise TypeError('data and offsets must both be torch tensors on the device, or both host buffers')
            for tensor, kinds in ((data, (torch.uint8,)), (offsets, (torch.int32, torch.uint32))):
                if tensor.device.type != 'cuda' or tensor.device.index != index or tensor.dtype not in kinds or not tensor.is_contiguous():
                    raise TypeError('device-resident words: contiguous uint8 bytes and int32 offsets on cuda:{}'.format(index))
            self._impl.packed_device_to_rows_device(
                data.data_ptr(), data.numel(), offsets.data_ptr(), n, out.data_ptr(), _current_stream(torch, index))
            return out
        offsets = host_offsets(offsets)
        batch = self._word_batches.take(index)
        try:
            self._impl.packed_to_rows_device(batch, data, offsets, out.data_ptr(), _current_stream(torch, index))
        finally:
            self._word_batches.give(batch)
        return out

    def batch_embedding_device(self, words, dtype=None):
        '''batch_embedding with the result left on the GPU as a torch.Tensor (DLPack capable). Words are resolved on
        the GPU as well (resolve_rows_device): the only host work is packing the strings. May be called from several
        threads at once. dtype: torch.float32 (default), torch.bfloat16 or torch.float16 (rows_embedding_device).'''
        return self.rows_embedding_device(self.resolve_rows_device(words), dtype=dtype)

    def rows_embedding_device_many(self, batches):
        '''Several lookups in ONE kernel launch (memb_hip_decode_batches_device): `batches` is a sequence of
        (rows, out) or (rows, out, col_off) with the tensors rows_embedding_device takes; results are those of one
        rows_embedding_device call per entry. For serving loops whose batches are too small to fill the GPU: launch gap,
        prologue and tail are paid once. Returns the list of `out` tensors.'''
        import torch
        index = self._impl.device()
        if index == _memb.HOST_DEVICE:
            raise RuntimeError("this reader decodes on the host (device 'cpu'): device buffers need a reader on a HIP device")
        descriptors = []
        outs = []
        for entry in batches:
            rows, out = entry[0], entry[1]
            col_off = entry[2] if len(entry) > 2 else 0
            if rows.device.type != 'cuda' or rows.dtype not in (torch.int32, torch.uint32) or not rows.is_contiguous():
                raise TypeError('rows must be a contiguous int32/uint32 tensor on the GPU')
            n = rows.numel()
            if out.dtype != torch.float32 or out.dim() != 2 or out.stride(1) != 1 or out.shape[0] != n:
                raise TypeError('out must be a float32 (n, width) tensor with unit column stride')
            if rows.device.index != index or out.device != rows.device:
                raise ValueError('rows and out must be on cuda:{} (the device this reader is staged on)'.format(self.device))
            if out.shape[1] < col_off + self.dim:
                raise ValueError('out is narrower than col_off + dim')
            descriptors.append((rows.data_ptr(), n, out.data_ptr(), out.stride(0) if n > 1 else out.shape[1], col_off))
            outs.append(out)
        self._impl.batches_to_device(descriptors, _current_stream(torch, index))
        return outs

    def tokenizer_embedding_device(self, tokenizer, dtype=None):
        '''tokenizer_embedding with the weights left on the GPU: a torch.Tensor that
        torch.nn.Embedding.from_pretrained (or any DLPack consumer) takes as is, so the
        embedding matrix of a model never crosses PCIe. dtype: as batch_embedding_device'''
        return self.batch_embedding_device(tokenizer_word_list(tokenizer), dtype=dtype)

    def info(self, batch_words=0):
        '''Facts about the device context (stages the model on first call). The kernel and its launch geometry
        are chosen by batch size: batch_words names the size they are reported for (0 = a large batch).'''
        return self._impl.info(int(batch_words))

    def set_option(self, name, value):
        '''Tuning knob of the device context ('persistent', 'tiles_per_wave', 'waves_per_block', 'union_split', 'union_fused',
        'host_expand': include/memb_hip.h, memb_hip_ctx_set_option); results never depend on them'''
        self._impl.set_option(str(name), int(value))
