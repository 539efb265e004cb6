"""Pooled unions without a GPU: the C header and entry points of include/memb_hip_pooled_union.h, and what the compiler
made of the kernels of memb_hip_pooled_union.hip (tools/perf/isa.py, source=POOLED_UNION_SOURCE)."""
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

HEADER = os.path.join(REPO, 'include', 'memb_hip_pooled_union.h')
needs_hipcc = pytest.mark.skipif(
    not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')), reason='hipcc not available')

KEY_FORMS = (('false', 'true'), ('false', 'false'), ('true', 'false'))   # <HAS_SUB, FAST>
# DESIGN.md section 5.6, "Pooled unions": what the fused instances may take, by their model count. LDS, not registers, is
# what bounds their residency (at most 20 wavefronts per CU, five per SIMD, for two models) as long as these hold.
VGPR_BOUND = {'2': 80, '3': 80, '4': 88}
WAVES_PER_SIMD = {'2': 6, '3': 6, '4': 5}


def test_header_is_plain_c_and_cxx():
    for compiler, flags in (('gcc', ['-std=c99', '-pedantic', '-Wall', '-Werror', '-x', 'c']),
                            ('g++', ['-std=c++14', '-Wall', '-Werror', '-x', 'c++'])):
        result = subprocess.run([compiler, *flags, '-fsyntax-only', HEADER], stdout=subprocess.PIPE,
                                stderr=subprocess.STDOUT, text=True)
        assert result.returncode == 0, result.stdout
    assert '#include "memb_hip_pooled.h"' in open(HEADER).read()
    # the headers it extends are as they were
    for name in ('memb_hip.h', 'memb_hip_pooled.h'):
        text = open(os.path.join(REPO, 'include', name)).read()
        assert 'memb_hip_pool_rows_union' not in text and 'memb_hip_pool_dense' not in text


def test_entry_points_are_exported_and_refuse_bad_arguments(native):
    library = ctypes.CDLL(native.HIP_LIBRARY_PATH)
    library.memb_hip_last_error.restype = ctypes.c_char_p
    fused = library.memb_hip_pool_rows_union_device
    fused.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_size_t,
                      ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    assert fused(None, None, 2, 0, None, 0, None, 0, 300, 0, 1, None) == 1   # MEMB_HIP_ERR_INVALID: no contexts
    assert b'null' in library.memb_hip_last_error()
    contexts = (ctypes.c_void_p * 2)(None, None)
    rows = (ctypes.c_void_p * 2)(None, None)
    assert fused(contexts, rows, 2, 0, None, 0, None, 0, 300, 0, 1, None) == 1   # null contexts in the array
    assert b'null' in library.memb_hip_last_error()
    assert fused(contexts, rows, 2, 0, None, 0, None, 0, 300, 0, 2, None) == 1
    assert b'pooling mode' in library.memb_hip_last_error()
    assert fused(contexts, rows, 2, 0, None, 0, None, 3, 300, 0, 1, None) == 1
    assert b'out_type' in library.memb_hip_last_error()
    dense = library.memb_hip_pool_dense_rows_device
    dense.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p,
                      ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    assert dense(0, None, 5, 300, 300, None, 0, None, 0, 300, 0, 1, None) == 1   # values missing
    assert b'null' in library.memb_hip_last_error()
    assert dense(0, None, 0, 300, 300, None, 4, None, 0, 300, 0, 1, None) == 1   # offsets and out missing
    assert b'null' in library.memb_hip_last_error()
    assert dense(0, None, 0, 0, 0, None, 0, None, 0, 300, 0, 1, None) == 1
    assert b'dim' in library.memb_hip_last_error()
    assert dense(0, None, 0, 300, 299, None, 0, None, 0, 300, 0, 1, None) == 1
    assert b'ld_values' in library.memb_hip_last_error()
    assert dense(0, None, 0, 300, 300, None, 0, None, 0, 299, 0, 1, None) == 1
    assert b'ld must be' in library.memb_hip_last_error()
    assert dense(0, None, 0, 300, 300, None, 0, None, 0, 300, 0, 5, None) == 1
    assert b'pooling mode' in library.memb_hip_last_error()
    assert dense(0, None, 0, 300, 300, None, 0, None, 0, 300, 0, 1, None) == 0   # bags == 0: a no-op
    name = library.memb_hip_pool_union_kernel_name
    name.restype = ctypes.c_char_p
    name.argtypes = [ctypes.c_void_p]
    assert name(None) == b''
    dense_name = library.memb_hip_pool_dense_kernel_name
    dense_name.restype = ctypes.c_char_p
    dense_name.argtypes = [ctypes.c_int]
    assert [dense_name(out_type) for out_type in (0, 1, 2, 3, -1)] == [b'pool_dense<0>', b'pool_dense<1>', b'pool_dense<2>', b'', b'']
    from memb_amd import _memb
    for binding in ('pool_union_rows_to_device', 'pool_union_kernel_name', 'pool_dense_rows_to_device', 'pool_dense_kernel_name'):
        assert hasattr(_memb, binding)
    assert native.POOLED_HOST_CHUNK == 1 << 16


def kernel_family(name):
    return name.split('(')[0].split('<')[0].split(' ')[-1]


def template_arguments(name):
    return name.split('<')[1].split('>')[0].split(', ')


@pytest.fixture(scope='module')
def unit():
    import isa
    return {name.replace('(anonymous namespace)::', ''): facts
            for name, facts in isa.kernel_table(source=isa.POOLED_UNION_SOURCE).items()}


@needs_hipcc
def test_the_unit_holds_the_fused_and_the_dense_kernels(unit):
    # three key forms x two to four models x three out types; one dense kernel per out type
    assert collections.Counter(kernel_family(name) for name in unit) == {'pool_trained_union': 27, 'pool_dense': 3}
    forms = sorted(tuple(template_arguments(name)) for name in unit if 'pool_trained_union<' in name)
    assert forms == sorted((has_sub, fast, count, out) for has_sub, fast in KEY_FORMS for count in '234' for out in '012')
    assert sorted(template_arguments(name)[0] for name in unit if 'pool_dense<' in name) == ['0', '1', '2']
    import isa
    assert isa.POOLED_UNION_SOURCE in isa.SOURCES


@needs_hipcc
def test_no_packed_fp32_no_scratch_no_atomics(unit):
    # the packed forms flush subnormals on gfx950: sums, the division by the model count (a
    # multiplication by 0.5 or 0.25 where it is a power of two) and the mean are single-lane operations
    for name, facts in unit.items():
        code = facts['code']
        assert not re.findall(r'^\s*v_pk_(?:add|mul|fma)_f32\s', code, flags=re.M), name
        assert facts['private_segment'] == 0 and facts['scratch_ops'] == 0, (name, facts['private_segment'])
        assert facts['load_nt'] == 0 and facts['store_nt'] == 0, name
        assert not re.findall(r'^\s*(?:global|flat|buffer|ds)_atomic_\w+\s', code, flags=re.M), name
        assert not re.findall(r'^\s*ds_\w+_rtn_\w+\s', code, flags=re.M), name
        stores = re.findall(r'^\s*(?:global|flat|buffer)_store_\w+\s.*$', code, flags=re.M)
        assert stores and not [line for line in stores if re.search(r'\b(sc0|sc1|nt)\b', line)], name
        assert not re.findall(r'^\s*v_(?:fmac|fma|mac)_f32\s.*;.*addRn', code, flags=re.M), name


@needs_hipcc
def test_fused_instances_add_one_lane_at_a_time_and_meet_the_register_bound(unit):
    import isa
    for name, facts in unit.items():
        if 'pool_trained_union<' not in name:
            continue
        _, _, count, out = template_arguments(name)
        # per merged piece COUNT - 1 adds of four, one more into the accumulator, for two pieces per lane
        assert len(re.findall(r'^\s*v_add_f32_e32\s', facts['code'], flags=re.M)) >= 8 * int(count), name
        if count in '24':
            assert len(re.findall(r'^\s*v_mul_f32_e32\s', facts['code'], flags=re.M)) >= 8, name
        assert facts['vgpr'] <= VGPR_BOUND[count], (name, facts['vgpr'])
        assert isa.waves_per_simd(facts['vgpr'], facts['sgpr_count']) >= WAVES_PER_SIMD[count], (name, facts['vgpr'], facts['sgpr_count'])
        stores = collections.Counter(re.findall(r'^\s*(?:global|flat|buffer)_store_(\w+)\s', facts['code'], flags=re.M))
        # fp32 pieces leave as 16-byte stores, bf16 / fp16 pieces as 8-byte stores of four elements
        if out == '0':
            assert stores['dwordx4'] >= 1, (name, stores)
        else:
            assert stores['dwordx2'] >= 1 and stores['dwordx4'] == 0 and stores['dwordx3'] == 0, (name, stores)


@needs_hipcc
def test_dense_kernels_hold_eight_wavefronts_per_simd(unit):
    import isa
    for name, facts in unit.items():
        if 'pool_dense<' in name:
            assert isa.waves_per_simd(facts['vgpr'], facts['sgpr_count']) == 8, (name, facts['vgpr'], facts['sgpr_count'])
            assert len(re.findall(r'^\s*v_add_f32_e32\s', facts['code'], flags=re.M)) >= 4, name
