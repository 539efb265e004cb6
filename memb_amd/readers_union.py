"""Several readers behind one reader's interface.

Interface and results of the reference's `memb.ReadersUnion`
(python/memb/readers_union.py:41-104): mode 'concatenate' lays the readers'
vectors side by side, mode 'average' takes their float32 mean; a word that one
reader does not know contributes zeros there. Differences are only in how the
rows get where they belong: for concatenation every reader decodes straight into
its column block of the result (the C ABI's `ld` / `col_off`), and
`batch_embedding_device` does either merge without leaving the GPU. Pooled lookups -- the sum or mean of each bag of
merged rows -- are `pooled_rows_device`, `pooled_sentences_device` and `pooled_rows`.
"""
import numpy as np

from .reader import (BaseReader, Reader, WordBatches, _current_stream, bag_offsets, flatten_sentences, pool_mode, pool_slices_host,
                     pooled_output, tokenizer_word_list)

CONCATENATE = 'concatenate'
AVERAGE = 'average'
MODES = (AVERAGE, CONCATENATE)
POOLED_HOST_CHUNK = 1 << 16   # entries pooled_rows of a union of device='cpu' readers decodes and merges at a time


def _merge_host(mode, pieces):
    """numpy merge of per-reader results (1-D vectors or 2-D batches)"""
    if mode == CONCATENATE:
        return np.concatenate(pieces, axis=-1)
    return np.mean(pieces, axis=0)


class ReadersUnion(BaseReader):
    """readers : at least two readers (for 'average' all of one dimension)
    mode    : 'average' or 'concatenate'
    `dim` is the dimension of the merged vectors."""

    def __init__(self, readers, mode):
        super().__init__()
        if len(readers) < 2:
            raise AssertionError('You must pass at least 2 readers to create a union')
        if mode not in MODES:
            raise KeyError('Mode {} is not supported. Available modes are {}'.format(mode, list(MODES)))
        widths = [reader.dim for reader in readers]
        if mode == AVERAGE and len(set(widths)) != 1:
            raise AssertionError('Dimensions of all readers must be equal for average mode')
        self._readers = list(readers)
        self._mode = mode
        self._widths = widths
        self._word_batches = WordBatches()   # of batch_embedding_device (one per call in flight), shared by the readers
        self._last_pooled_kernel = ''

    @property
    def dim(self):
        return sum(self._widths) if self._mode == CONCATENATE else self._widths[0]

    def keys(self):
        """Every word at least one reader knows, sorted"""
        merged = set()
        for reader in self._readers:
            merged.update(reader.keys())
        return sorted(merged)

    def word_embedding(self, word):
        return _merge_host(self._mode, [reader.word_embedding(word) for reader in self._readers])

    def batch_embedding(self, words):
        native = all(isinstance(reader, Reader) for reader in self._readers)
        if self._mode == CONCATENATE and native:
            # no concatenation pass: each reader fills its own columns of the result
            merged = np.empty((len(words), self.dim), dtype=np.float32)
            column = 0
            for reader, width in zip(self._readers, self._widths):
                reader.batch_embedding_into(words, merged, column)
                column += width
            return merged
        return _merge_host(self._mode, [reader.batch_embedding(words) for reader in self._readers])

    def _device_index(self):
        """The HIP device every reader is staged on; refuses unions the device methods cannot serve"""
        readers = self._readers
        if not all(isinstance(reader, Reader) for reader in readers):
            raise TypeError('device merge needs memb_amd.Reader instances')
        if len({reader.device for reader in readers}) != 1:
            raise ValueError('all readers of a union must be on one device')
        from . import _memb
        index = readers[0]._impl.device()
        if index == _memb.HOST_DEVICE:
            raise RuntimeError("these readers decode on the host (device 'cpu'): device buffers need readers on a HIP device")
        return index

    def resolve_rows_device(self, words):
        """The row ids of `words` in every reader, left on the GPU: a list of R torch.int32 tensors (views of the uint32
        ids, 0xFFFFFFFF where a reader does not know a word), each equal to that reader's own resolve_rows_device. The
        words are packed and copied ONCE and resolved by every reader's own hash table: the ids never visit the host.
        May be called from several threads at once."""
        import torch
        from . import _memb
        readers = self._readers
        index = self._device_index()
        device = 'cuda:{}'.format(index)
        stream = torch.cuda.current_stream(torch.device(device)).cuda_stream
        row_ids = [torch.empty((len(words),), dtype=torch.int32, device=device) for _ in readers]
        batch = self._word_batches.take(index)
        try:
            _memb.union_words_to_rows_device(
                batch, words, [reader._impl for reader in readers], [ids.data_ptr() for ids in row_ids], stream)
        finally:
            self._word_batches.give(batch)
        return row_ids

    def _merge_rows_device(self, row_ids, merged, stream):
        """The merged float32 rows of one row-id tensor per reader into `merged` (n, dim), n > 0: one launch that decodes
        every reader's words of a tile and writes the merged rows once, where the readers can share a kernel"""
        from . import _memb
        readers = self._readers
        n = merged.shape[0]
        concatenate = self._mode == CONCATENATE
        columns = [sum(self._widths[:i]) if concatenate else 0 for i in range(len(readers))]
        if _memb.union_rows_to_device(
                [reader._impl for reader in readers], [ids.data_ptr() for ids in row_ids], columns,
                n, merged.data_ptr(), merged.stride(0), stream, not concatenate):
            return merged
        if concatenate:
            column = 0
            for reader, ids, width in zip(readers, row_ids, self._widths):
                reader.rows_embedding_device(ids, out=merged, col_off=column)
                column += width
            return merged
        count = len(readers)
        for position, (reader, ids) in enumerate(zip(readers, row_ids)):
            reader.rows_embedding_device(
                ids, out=merged, accumulate=position > 0, divisor=float(count) if position == count - 1 else 0.0)
        return merged

    def batch_embedding_device(self, words):
        """batch_embedding merged on the GPU, returned as a torch.Tensor (not in the
        reference API). Concatenation: column blocks of one (n, dim) tensor. Average:
        reader 1 stores, readers 2..R add, the last one also divides by R -- the very
        additions and the one division numpy.mean performs, in its order, so the
        result has the same bits as batch_embedding. All readers on one device. May be called from several threads
        at once."""
        import torch
        device = 'cuda:{}'.format(self._device_index())
        stream = torch.cuda.current_stream(torch.device(device)).cuda_stream
        row_ids = self.resolve_rows_device(words)
        merged = torch.empty((len(words), self.dim), dtype=torch.float32, device=device)
        if len(words):
            self._merge_rows_device(row_ids, merged, stream)
        return merged

    def bags_embedding_device(self, *args, **kwargs):
        """A union's bag is of ENTRIES of one row id per reader, which the one-array signature of
        Reader.bags_embedding_device has no place for: see pooled_rows_device, pooled_sentences_device and pooled_rows"""
        raise NotImplementedError(
            'a ReadersUnion pools entries of one row id per reader: use pooled_rows_device, pooled_sentences_device or pooled_rows')

    bags_embedding = sentences_embedding_device = bags_embedding_device

    @property
    def last_pooled_kernel(self):
        """The kernel the last 'average' pooled launch of this union ran -- 'pool_trained_union<..>' for the fused kernel,
        'pool_dense<..>' for the fallback over merged rows, both as the library names them -- or '' before any.
        Informational, like info()['union_kernel']: with several threads in pooled_rows_device it is the kernel of whichever
        call recorded it last."""
        return self._last_pooled_kernel

    def pooled_rows_device(self, rows, offsets, mode='mean', out=None, col_off=0, dtype=None):
        """Pooled lookup of merged rows that never leaves the GPU: the sum or mean of each bag of the rows
        batch_embedding_device writes, bit for bit Reader.bags_embedding_device's loop over them.
        Parameters
        ----------
        rows : a sequence of R contiguous int32 / uint32 torch.Tensors of equal length n on the readers' device, one per
            reader (resolve_rows_device): entry i is (rows[0][i], .., rows[R - 1][i]), a row a reader does not have
            (0xFFFFFFFF or an id >= len(reader)) is +0.0 there
        offsets, mode, out, col_off, dtype : as in Reader.bags_embedding_device; out is (bags, >= col_off + union.dim)
        'concatenate': every reader pools into its own column block, R launches of Reader.bags_embedding_device's kernels.
        'average': the merged row of an entry is (((v1 + v2) + ..) / R in float32. Trained readers of one dim (a multiple
        of 4, at most 512) and lane geometry with a 16-byte aligned `out` run ONE kernel that decodes every reader's rows,
        merges and adds them in registers: neither the readers' rows nor the merged rows are written. Every other averaged
        union -- uniform or full storage, mixed storages, other dims, more than four readers, an unaligned `out`, option
        union_fused = 0 on the first reader -- merges the rows into a float32 (n, dim) temporary of this call (4 n dim
        bytes) and pools that: the same bits. last_pooled_kernel says which ran.
        No missing='skip', no chunked reduction, no accumulate, weights or 'max'.
        May be called from several threads at once: nothing is shared between calls but last_pooled_kernel.
        """
        import torch
        from . import _memb
        code = pool_mode(mode)
        readers = self._readers
        index = self._device_index()
        if not isinstance(rows, (list, tuple)) or len(rows) != len(readers):
            raise ValueError('rows must be a sequence of one row-id tensor per reader ({})'.format(len(readers)))
        for ids in rows:
            if (not isinstance(ids, torch.Tensor) or ids.device.type != 'cuda' or ids.dtype not in (torch.int32, torch.uint32)
                    or not ids.is_contiguous()):
                raise TypeError('rows must be contiguous int32/uint32 tensors on the GPU')
        n = rows[0].numel()
        if any(ids.numel() != n for ids in rows):
            raise ValueError('the row-id tensors of a union must be of equal length')
        device = rows[0].device

        def check_devices(out):
            if (device.index != index or out.device != device or offsets.device != device
                    or any(ids.device != device for ids in rows)):
                raise ValueError('rows, offsets and out must be on cuda:{} (the device these readers are staged on), got {}, {} and {}'.format(
                    index, sorted({str(ids.device) for ids in rows}), offsets.device, out.device))

        dim = self.dim
        bags, out, out_type, ld = pooled_output(torch, offsets, out, dtype, col_off, dim, device, check_devices)
        if self._mode == CONCATENATE:
            column = col_off
            for reader, ids, width in zip(readers, rows, self._widths):
                reader.bags_embedding_device(ids, offsets, mode=mode, out=out, col_off=column, dtype=dtype)
                column += width
            return out
        if bags == 0:
            return out
        stream = _current_stream(torch, index)
        if _memb.pool_union_rows_to_device(
                [reader._impl for reader in readers], [ids.data_ptr() for ids in rows], n, offsets.data_ptr(), bags,
                out.data_ptr(), ld, col_off, code, stream, out_type):
            self._last_pooled_kernel = _memb.pool_union_kernel_name(readers[0]._impl)
            return out
        # this call's own: torch's allocator keeps it alive for the work enqueued on the current stream
        merged = torch.empty((n, dim), dtype=torch.float32, device=device)
        if n:
            self._merge_rows_device(list(rows), merged, stream)
        _memb.pool_dense_rows_to_device(
            index, merged.data_ptr(), n, dim, dim, offsets.data_ptr(), bags, out.data_ptr(), ld, col_off, code, stream, out_type)
        self._last_pooled_kernel = _memb.pool_dense_kernel_name(out_type)
        return out

    def pooled_sentences_device(self, sentences, mode='mean', dtype=None):
        """One merged vector per sentence, left on the GPU: `sentences` is a sequence of word sequences; the words are
        resolved on the device by every reader (resolve_rows_device) and each sentence's merged rows are pooled by
        pooled_rows_device. A sentence without words is a zero vector. Returns a (len(sentences), dim) tensor of `dtype`."""
        import torch
        pool_mode(mode)
        index = self._device_index()
        words, offsets = flatten_sentences(sentences)
        device = 'cuda:{}'.format(index)
        if words:
            rows = self.resolve_rows_device(words)
        else:
            rows = [torch.empty((0,), dtype=torch.int32, device=device) for _ in self._readers]
        on_device = torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).to(device)
        return self.pooled_rows_device(rows, on_device, mode=mode, dtype=dtype)

    def pooled_rows(self, rows, offsets, mode='mean'):
        """pooled_rows_device for host arrays: a sequence of R numpy row-id arrays of equal length and offsets in, a numpy
        float32 (bags, dim) matrix out. offsets: bags + 1 integers, ascending, within 0 .. n -- anything else is a
        ValueError. Readers on a GPU send the ids and offsets up and bring only bags x dim floats back. A union of
        device='cpu' readers decodes rows_embedding in slices of POOLED_HOST_CHUNK entries, merges them in numpy float32 in
        pooled_rows_device's order and adds them in entry order: the same bits."""
        code = pool_mode(mode)
        readers = self._readers
        if not all(isinstance(reader, Reader) for reader in readers):
            raise TypeError('pooled lookups need memb_amd.Reader instances')
        if isinstance(rows, np.ndarray) and rows.ndim == 1 or len(rows) != len(readers):
            raise ValueError('rows must be a sequence of one row-id array per reader ({})'.format(len(readers)))
        rows = [np.ascontiguousarray(ids, dtype=np.uint32).reshape(-1) for ids in rows]
        n = rows[0].size
        if any(ids.size != n for ids in rows):
            raise ValueError('the row-id arrays of a union must be of equal length')
        offsets = bag_offsets(offsets, n)
        from . import _memb
        on_host = [reader._impl.device() == _memb.HOST_DEVICE for reader in readers]
        if not any(on_host):
            import torch
            device = 'cuda:{}'.format(self._device_index())
            result = self.pooled_rows_device(
                [torch.from_numpy(ids.view(np.int32)).to(device) for ids in rows],
                torch.from_numpy(offsets.astype(np.uint32).view(np.int32)).to(device), mode=mode)
            return result.cpu().numpy()
        if not all(on_host):
            raise ValueError('all readers of a union must be on one device')

        def slice_values(start, stop):
            pieces = [reader.rows_embedding(ids[start:stop]) for reader, ids in zip(readers, rows)]
            if self._mode == CONCATENATE:
                values = np.hstack(pieces)
            else:
                values = pieces[0]
                for piece in pieces[1:]:
                    values = np.add(values, piece, dtype=np.float32)
                values = np.divide(values, np.float32(len(readers)), dtype=np.float32)
            yield values

        return pool_slices_host(offsets, n, self.dim, POOLED_HOST_CHUNK, code == _memb.POOL_MEAN, False, slice_values)[0]

    def tokenizer_embedding(self, tokenizer):
        """Embedding-layer weights for a keras Tokenizer, merged over the readers"""
        return self.batch_embedding(tokenizer_word_list(tokenizer))

    def tokenizer_embedding_device(self, tokenizer):
        """tokenizer_embedding merged on the GPU (see batch_embedding_device)"""
        return self.batch_embedding_device(tokenizer_word_list(tokenizer))
