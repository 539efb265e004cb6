"""bf16 / fp16 rows without a GPU: the C header and entry point of include/memb_hip_narrow.h, and what the compiler made of
the kernels of memb_hip_narrow.hip (tools/perf/isa.py, source=NARROW_SOURCE)."""
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

HEADER = os.path.join(REPO, 'include', 'memb_hip_narrow.h')
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
    assert {name: int(value) for name, value in re.findall(r'#define (MEMB_HIP_OUT_\w+) (\d+)', text)} == {
        'MEMB_HIP_OUT_F32': 0, 'MEMB_HIP_OUT_BF16': 1, 'MEMB_HIP_OUT_F16': 2}


def test_typed_entry_is_exported_and_refuses_bad_arguments(native):
    library = ctypes.CDLL(native.HIP_LIBRARY_PATH)
    library.memb_hip_last_error.restype = ctypes.c_char_p
    typed = library.memb_hip_decode_rows_device_typed
    typed.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int,
                      ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p]
    for out_type in (0, 1, 2):
        assert typed(None, None, 0, None, out_type, 300, 0, None) == 1   # MEMB_HIP_ERR_INVALID: no context
        assert b'null' in library.memb_hip_last_error()
    for out_type in (-1, 3, 16):
        assert typed(None, None, 0, None, out_type, 300, 0, None) == 1
        assert b'out_type' in library.memb_hip_last_error()
    from memb_amd import _memb
    assert (_memb.OUT_F32, _memb.OUT_BF16, _memb.OUT_F16) == (0, 1, 2)


@pytest.fixture(scope='module')
def kernels():
    import isa
    return {name.replace('(anonymous namespace)::', ''): facts for name, facts in isa.kernel_table(source=isa.NARROW_SOURCE).items()}


@needs_hipcc
def test_the_narrow_kernel_families(kernels):
    # decode_trained_narrow: three key forms x three output modes (SCALAR, VEC4, FLAT) x two element types; the row-wise
    # kernels VEC4 x two types. Nothing else: the staging kernels stay in memb_hip.hip alone.
    families = collections.Counter(name.split(' ', 1)[1].split('<')[0] for name in kernels)
    assert families == {'decode_trained_narrow': 18, 'dequant_uniform_narrow': 4, 'gather_full_narrow': 4}, families


@needs_hipcc
def test_narrow_kernels_spill_nothing_and_store_plainly(kernels):
    import isa
    for name, facts in kernels.items():
        assert facts['private_segment'] == 0 and facts['scratch_ops'] == 0, (name, facts)
        assert facts['load_nt'] == 0 and facts['store_nt'] == 0, (name, facts)
    text = isa.device_assembly(source=isa.NARROW_SOURCE)
    stores = re.findall(r'^\s*(?:global|flat|buffer)_store_\w+\s.*$', text, flags=re.M)
    assert stores and not [line for line in stores if re.search(r'\b(sc0|sc1|nt)\b', line)]


@needs_hipcc
def test_dense_rows_leave_in_16_byte_stores(kernels):
    # OUT_FLAT (mode 2): eight values per lane and store; the row-by-row modes never use 16 bytes
    for name, facts in kernels.items():
        if 'decode_trained_narrow<' in name:
            mode = int(name.split('<')[1].split(',')[1])
            assert (facts['store_x4'] >= 1) == (mode == 2), (name, facts)


@needs_hipcc
def test_narrow_kernels_keep_the_one_tile_residency(kernels):
    # hip_decode_plan.h plans decode_trained_narrow with ONE_TILE_WAVES_PER_CU = 28, as decode_trained: seven per SIMD
    import isa
    for name, facts in kernels.items():
        if 'decode_trained_narrow<' in name:
            assert isa.waves_per_simd(facts['vgpr'], facts['sgpr_count']) == 7, (name, facts)


def test_narrow_conversion_is_a_plain_cast():
    # the integer round-to-nearest-even form turns some NaNs into zeros or infinities: not used
    source = open(os.path.join(REPO, 'memb_amd', 'csrc', 'hip_device_common.h')).read()
    body = source[source.index('uint32_t narrowBits'):]
    body = body[:body.index('\n}\n')]
    assert 'static_cast<__bf16>(value)' in body and 'static_cast<_Float16>(value)' in body and '0x7FFF' not in body
