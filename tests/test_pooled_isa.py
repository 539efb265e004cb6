"""Pooled lookups without a GPU: the C header and entry points of include/memb_hip_pooled.h, and what the compiler made of
the kernels of memb_hip_pooled.hip (tools/perf/isa.py, source=POOLED_SOURCE), family by family: the fp32 kernels, their
bf16 / fp16 forms and the kernels that skip missing rows."""
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


KEY_FORMS = (('false', 'true'), ('false', 'false'), ('true', 'false'))   # <HAS_SUB, FAST>
# family: the trained kernel (the row-wise ones are named alike), its out types as template arguments (None: fp32, not a
# template argument), the least v_add_f32_e32 its code must hold
FAMILIES = {
    'fp32': ('pool_trained', None, 8),
    'narrow': ('pool_trained_narrow', ('1', '2'), 16),
    'known': ('pool_known_trained', ('0', '1', '2'), 24),
}


def family_names(family):
    trained = FAMILIES[family][0]
    return trained, trained.replace('trained', 'uniform'), trained.replace('trained', 'full')


def kernel_family(name):
    return name.split('(')[0].split('<')[0].split(' ')[-1]


def template_arguments(name):
    return name.split('<')[1].split('>')[0].split(', ')


@pytest.fixture(scope='module')
def unit():
    import isa
    return {name.replace('(anonymous namespace)::', ''): facts for name, facts in isa.kernel_table(source=isa.POOLED_SOURCE).items()}


@pytest.fixture(params=sorted(FAMILIES))
def family(request):
    return request.param


@pytest.fixture
def kernels(unit, family):
    return {name: facts for name, facts in unit.items() if kernel_family(name) in family_names(family)}


@pytest.fixture
def code(kernels):
    return '\n'.join(facts['code'] for facts in kernels.values())


@needs_hipcc
def test_the_unit_holds_the_three_families_and_nothing_else(unit):
    # the staging kernels stay in memb_hip.hip alone, the chunked order's in memb_hip_pooled_chunked.hip
    assert {kernel_family(name) for name in unit} == {name for family in FAMILIES for name in family_names(family)}
    assert len(unit) == 8 + 16 + 24


@needs_hipcc
def test_the_pooled_kernel_families(kernels, family):
    # trained: three key forms x (column form, pieces) x the family's out types; one row-wise kernel per other storage and type
    trained, uniform, full = family_names(family)
    outs = FAMILIES[family][1]
    types = len(outs or (None,))
    assert collections.Counter(kernel_family(name) for name in kernels) == {trained: 6 * types, uniform: types, full: types}
    forms = sorted(tuple(template_arguments(name)) for name in kernels if trained + '<' in name)
    assert forms == sorted((has_sub, fast, vec4) + ((out,) if outs else ()) for has_sub, fast in KEY_FORMS
                           for vec4 in ('false', 'true') for out in outs or (None,)), forms
    for rowwise in (uniform, full) if outs else ():
        assert sorted(template_arguments(name)[0] for name in kernels if rowwise + '<' in name) == list(outs)


@needs_hipcc
def test_pooled_kernels_spill_nothing_and_store_plainly(kernels, code):
    for name, facts in kernels.items():
        assert facts['private_segment'] == 0 and facts['scratch_ops'] == 0, (name, facts)
        assert facts['load_nt'] == 0 and facts['store_nt'] == 0, (name, facts)
    stores = re.findall(r'^\s*(?:global|flat|buffer)_store_\w+\s.*$', code, flags=re.M)
    assert stores and not [line for line in stores if re.search(r'\b(sc0|sc1|nt)\b', line)]
    # no atomics: the result is a function of the inputs alone
    assert not re.findall(r'^\s*(?:global|flat|buffer|ds)_atomic_\w+\s', code, flags=re.M)
    assert not re.findall(r'^\s*ds_\w+_rtn_\w+\s', code, flags=re.M)


@needs_hipcc
def test_every_accumulator_add_is_a_single_lane_op(code, family):
    # the packed forms flush subnormals on gfx950: the sums are v_add_f32 only
    assert not re.findall(r'^\s*v_pk_(?:add|mul|fma)_f32\s', code, flags=re.M)
    assert len(re.findall(r'^\s*v_add_f32_e32\s', code, flags=re.M)) >= FAMILIES[family][2]
    assert not re.findall(r'^\s*v_(?:fmac|fma|mac)_f32\s.*;.*addRn', code, flags=re.M)


@needs_hipcc
def test_trained_pooled_kernels_keep_the_one_tile_residency_and_their_store_widths(kernels, family):
    # hip_decode_plan.h plans every trained kernel like decode_trained, with ONE_TILE_WAVES_PER_CU = 28: seven wavefronts per SIMD
    # was planned for (eight accumulator registers on top of the decode's), and seven is what the compiler gave.
    # fp32: the piece form leaves as 16-byte stores. bf16 / fp16: as 8-byte stores of four elements, and the column form --
    # any alignment -- as single elements only.
    import isa
    trained = family_names(family)[0]
    instances = {name: facts for name, facts in kernels.items() if trained + '<' in name}
    assert len(instances) == 6 * len(FAMILIES[family][1] or (None,))
    for name, facts in instances.items():
        assert isa.waves_per_simd(facts['vgpr'], facts['sgpr_count']) == 7, (name, facts)
        vec4 = template_arguments(name)[2] == 'true'
        stores = collections.Counter(re.findall(r'^\s*(?:global|flat|buffer)_store_(\w+)\s', facts['code'], flags=re.M))
        if family == 'fp32':
            assert (facts['store_x4'] >= 1) == vec4, (name, facts)
        elif family == 'narrow':
            assert (stores['dwordx2'] >= 1) == vec4, (name, stores)
            assert facts['store_x4'] == 0 and stores['dwordx3'] == 0, (name, stores)
            if not vec4:
                assert set(stores) == {'short'}, (name, stores)
