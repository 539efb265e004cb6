"""bf16 / fp16 pooled lookups without a GPU: the typed entry points of include/memb_hip_pooled.h. What the compiler made of
their kernels: tests/test_pooled_isa.py, the family 'narrow'."""
import ctypes
import inspect
import os
import re
import subprocess

from conftest import REPO

HEADER = os.path.join(REPO, 'include', 'memb_hip_pooled.h')


def test_header_is_plain_c_and_cxx_and_declares_the_typed_calls():
    for compiler, flags in (('gcc', ['-std=c99', '-pedantic', '-Wall', '-Werror', '-x', 'c']),
                            ('g++', ['-std=c++14', '-Wall', '-Werror', '-x', 'c++'])):
        result = subprocess.run([compiler, *flags, '-fsyntax-only', HEADER], stdout=subprocess.PIPE,
                                stderr=subprocess.STDOUT, text=True)
        assert result.returncode == 0, result.stdout
    text = open(HEADER).read()
    assert 'memb_hip_pool_rows_device_typed' in text and 'memb_hip_pooled_algorithmic_bytes_typed' in text
    # the element types are memb_hip_narrow.h's: no new pooling define
    assert '#include "memb_hip_narrow.h"' in text and 'define MEMB_HIP_OUT_' not in text
    assert {name: int(value) for name, value in re.findall(r'#define (MEMB_HIP_POOL_\w+) (\d+)', text)} == {
        'MEMB_HIP_POOL_SUM': 0, 'MEMB_HIP_POOL_MEAN': 1}
    assert 'memb_hip_pool' not in open(os.path.join(REPO, 'include', 'memb_hip.h')).read()


def test_typed_entries_are_exported_and_refuse_bad_arguments(native):
    library = ctypes.CDLL(native.HIP_LIBRARY_PATH)
    library.memb_hip_last_error.restype = ctypes.c_char_p
    pool = library.memb_hip_pool_rows_device_typed
    pool.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                     ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    counted = library.memb_hip_pooled_algorithmic_bytes_typed
    counted.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int,
                        ctypes.c_void_p]
    for out_type in (0, 1, 2):
        for mode in (0, 1):
            assert pool(None, None, 0, None, 0, None, out_type, 300, 0, mode, None) == 1   # MEMB_HIP_ERR_INVALID: no context
            assert b'null' in library.memb_hip_last_error()
        assert pool(None, None, 0, None, 0, None, out_type, 300, 0, 2, None) == 1
        assert b'pooling mode' in library.memb_hip_last_error()
        assert counted(None, None, 0, None, 0, out_type, None) == 1
        assert b'null' in library.memb_hip_last_error()
    for out_type in (-1, 3, 7):
        assert pool(None, None, 0, None, 0, None, out_type, 300, 0, 0, None) == 1
        assert b'out_type' in library.memb_hip_last_error()
        assert counted(None, None, 0, None, 0, out_type, None) == 1
        assert b'out_type' in library.memb_hip_last_error()
    from memb_amd import _memb
    assert 'out_type' in _memb.Reader.pool_rows_to_device.__doc__
    assert 'out_type' in _memb.Reader.pooled_algorithmic_bytes.__doc__
    from memb_amd.reader import Reader
    for method in (Reader.bags_embedding_device, Reader.sentences_embedding_device):
        assert inspect.signature(method).parameters['dtype'].default is None
    assert 'dtype' not in inspect.signature(Reader.bags_embedding).parameters   # the numpy entry point stays float32
