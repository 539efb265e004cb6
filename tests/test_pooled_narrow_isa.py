"""bf16 / fp16 pooled lookups without a GPU: the typed entry points of include/memb_hip_pooled.h, and what the compiler made
of the kernels of memb_hip_pooled_narrow.hip (tools/perf/isa.py, source=POOLED_NARROW_SOURCE)."""
import collections
import ctypes
import inspect
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, 'tools', 'perf'))

HEADER = os.path.join(REPO, 'include', 'memb_hip_pooled.h')
needs_hipcc = pytest.mark.skipif(
    not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')), reason='hipcc not available')


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


@pytest.fixture(scope='module')
def kernels():
    import isa
    return {name.replace('(anonymous namespace)::', ''): facts
            for name, facts in isa.kernel_table(source=isa.POOLED_NARROW_SOURCE).items()}


def template_arguments(name):
    return name.split('<')[1].split('>')[0].split(', ')


@needs_hipcc
def test_the_narrow_pooled_kernel_families(kernels):
    # pool_trained_narrow: three key forms x (column form, 8-byte pieces) x (bf16, fp16); the row-wise kernels per type
    families = collections.Counter(name.split('(')[0].split('<')[0].split(' ')[-1] for name in kernels)
    assert families == {'pool_trained_narrow': 12, 'pool_uniform_narrow': 2, 'pool_full_narrow': 2}, families
    forms = sorted(tuple(template_arguments(name)) for name in kernels if 'pool_trained_narrow<' in name)
    assert forms == sorted((has_sub, fast, vec4, out) for has_sub, fast in
                           (('false', 'true'), ('false', 'false'), ('true', 'false'))
                           for vec4 in ('false', 'true') for out in ('1', '2')), forms
    for family in ('pool_uniform_narrow', 'pool_full_narrow'):
        assert sorted(template_arguments(name)[0] for name in kernels if family + '<' in name) == ['1', '2']


@needs_hipcc
def test_narrow_pooled_kernels_spill_nothing_and_store_plainly(kernels):
    import isa
    for name, facts in kernels.items():
        assert facts['private_segment'] == 0 and facts['scratch_ops'] == 0, (name, facts)
        assert facts['load_nt'] == 0 and facts['store_nt'] == 0, (name, facts)
    text = isa.device_assembly(source=isa.POOLED_NARROW_SOURCE)
    stores = re.findall(r'^\s*(?:global|flat|buffer)_store_\w+\s.*$', text, flags=re.M)
    assert stores and not [line for line in stores if re.search(r'\b(sc0|sc1|nt)\b', line)]
    # no atomics: the result is a function of the inputs alone
    assert not re.findall(r'^\s*(?:global|flat|buffer|ds)_atomic_\w+\s', text, flags=re.M)
    assert not re.findall(r'^\s*ds_\w+_rtn_\w+\s', text, flags=re.M)
    # the sums are single-lane v_add_f32: the packed forms flush subnormals on gfx950
    assert not re.findall(r'^\s*v_pk_(?:add|mul|fma)_f32\s', text, flags=re.M)
    assert len(re.findall(r'^\s*v_add_f32_e32\s', text, flags=re.M)) >= 16


@needs_hipcc
def test_narrow_trained_kernels_keep_the_one_tile_residency_and_their_store_widths(kernels):
    # launchPooled plans them like pool_trained, with ONE_TILE_WAVES_PER_CU = 28: seven wavefronts per SIMD. The piece form
    # leaves as 8-byte stores of four elements; the column form -- any alignment -- as single elements only.
    import isa
    text = isa.device_assembly(source=isa.POOLED_NARROW_SOURCE)
    for name, facts in kernels.items():
        if 'pool_trained_narrow<' not in name:
            continue
        assert isa.waves_per_simd(facts['vgpr'], facts['sgpr_count']) == 7, (name, facts)
        start = text.index('\n' + facts['symbol'] + ':')
        code = text[start:text.index('.amdhsa_kernel ' + facts['symbol'], start)].split('.section')[0]
        stores = collections.Counter(re.findall(r'^\s*(?:global|flat|buffer)_store_(\w+)\s', code, flags=re.M))
        vec4 = template_arguments(name)[2] == 'true'
        assert (stores['dwordx2'] >= 1) == vec4, (name, stores)
        assert facts['store_x4'] == 0 and stores['dwordx3'] == 0, (name, stores)
        if not vec4:
            assert set(stores) == {'short'}, (name, stores)
