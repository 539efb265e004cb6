"""Pooled lookups without a GPU: the C header and entry points of include/memb_hip_pooled.h, and what the compiler made of
the kernels of memb_hip_pooled.hip (tools/perf/isa.py, source=POOLED_SOURCE)."""
import collections
import ctypes
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


def test_header_is_plain_c_and_cxx():
    for compiler, flags in (('gcc', ['-std=c99', '-pedantic', '-Wall', '-Werror', '-x', 'c']),
                            ('g++', ['-std=c++14', '-Wall', '-Werror', '-x', 'c++'])):
        result = subprocess.run([compiler, *flags, '-fsyntax-only', HEADER], stdout=subprocess.PIPE,
                                stderr=subprocess.STDOUT, text=True)
        assert result.returncode == 0, result.stdout
    text = open(HEADER).read()
    assert '#include "memb_hip.h"' in text
    assert {name: int(value) for name, value in re.findall(r'#define (MEMB_HIP_POOL_\w+) (\d+)', text)} == {
        'MEMB_HIP_POOL_SUM': 0, 'MEMB_HIP_POOL_MEAN': 1}
    # memb_hip.h and its ABI version are as they were: the pooled call is an extension beside it
    assert 'memb_hip_pool' not in open(os.path.join(REPO, 'include', 'memb_hip.h')).read()


def test_pooled_entry_is_exported_and_refuses_bad_arguments(native):
    library = ctypes.CDLL(native.HIP_LIBRARY_PATH)
    library.memb_hip_last_error.restype = ctypes.c_char_p
    pool = library.memb_hip_pool_rows_device
    pool.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p,
                     ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    for mode in (0, 1):
        assert pool(None, None, 0, None, 0, None, 300, 0, mode, None) == 1   # MEMB_HIP_ERR_INVALID: no context
        assert b'null' in library.memb_hip_last_error()
        assert pool(None, None, 0, None, 4, None, 300, 0, mode, None) == 1
        assert b'null' in library.memb_hip_last_error()
    for mode in (-1, 2, 7):
        assert pool(None, None, 0, None, 0, None, 300, 0, mode, None) == 1
        assert b'pooling mode' in library.memb_hip_last_error()
    counted = library.memb_hip_pooled_algorithmic_bytes
    counted.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    assert counted(None, None, 0, None, 0, None) == 1
    assert b'null' in library.memb_hip_last_error()
    from memb_amd import _memb
    assert (_memb.POOL_SUM, _memb.POOL_MEAN) == (0, 1)
    assert hasattr(_memb.Reader, 'pool_rows_to_device')


@pytest.fixture(scope='module')
def kernels():
    import isa
    return {name.replace('(anonymous namespace)::', ''): facts for name, facts in isa.kernel_table(source=isa.POOLED_SOURCE).items()}


@needs_hipcc
def test_the_pooled_kernel_families(kernels):
    # pool_trained: three key forms x (column form, 16-byte pieces); one row-wise kernel per other storage. Nothing else:
    # the staging kernels stay in memb_hip.hip alone.
    families = collections.Counter(name.split('(')[0].split('<')[0].split(' ')[-1] for name in kernels)
    assert families == {'pool_trained': 6, 'pool_uniform': 1, 'pool_full': 1}, families
    forms = sorted(name.split('<')[1].split('>')[0] for name in kernels if 'pool_trained<' in name)
    assert forms == sorted('{}, {}, {}'.format(has_sub, fast, vec4) for has_sub, fast in
                           (('false', 'true'), ('false', 'false'), ('true', 'false')) for vec4 in ('false', 'true')), forms


@needs_hipcc
def test_pooled_kernels_spill_nothing_and_store_plainly(kernels):
    import isa
    for name, facts in kernels.items():
        assert facts['private_segment'] == 0 and facts['scratch_ops'] == 0, (name, facts)
        assert facts['load_nt'] == 0 and facts['store_nt'] == 0, (name, facts)
    text = isa.device_assembly(source=isa.POOLED_SOURCE)
    stores = re.findall(r'^\s*(?:global|flat|buffer)_store_\w+\s.*$', text, flags=re.M)
    assert stores and not [line for line in stores if re.search(r'\b(sc0|sc1|nt)\b', line)]
    # no atomics: the result is a function of the inputs alone
    assert not re.findall(r'^\s*(?:global|flat|buffer|ds)_atomic_\w+\s', text, flags=re.M)
    assert not re.findall(r'^\s*ds_\w+_rtn_\w+\s', text, flags=re.M)


@needs_hipcc
def test_every_accumulator_add_is_a_single_lane_op():
    # the packed forms flush subnormals on gfx950: the sums are v_add_f32 only
    import isa
    text = isa.device_assembly(source=isa.POOLED_SOURCE)
    assert not re.findall(r'^\s*v_pk_(?:add|mul|fma)_f32\s', text, flags=re.M)
    assert len(re.findall(r'^\s*v_add_f32_e32\s', text, flags=re.M)) >= 8
    assert not re.findall(r'^\s*v_(?:fmac|fma|mac)_f32\s.*;.*addRn', text, flags=re.M)


@needs_hipcc
def test_trained_pooled_kernels_keep_the_one_tile_residency(kernels):
    # memb_hip.hip plans pool_trained like decode_trained, with ONE_TILE_WAVES_PER_CU = 28: seven per SIMD was planned for
    # (eight accumulator registers on top of the decode's), and seven is what the compiler gave
    import isa
    for name, facts in kernels.items():
        if 'pool_trained<' in name:
            assert isa.waves_per_simd(facts['vgpr'], facts['sgpr_count']) == 7, (name, facts)
            vec4 = name.split('<')[1].split('>')[0].split(', ')[2] == 'true'
            assert (facts['store_x4'] >= 1) == vec4, (name, facts)
