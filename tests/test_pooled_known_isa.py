"""What the compiler made of the kernels of memb_hip_pooled_known.hip (tools/perf/isa.py, source=POOLED_KNOWN_SOURCE): the
checks tests/test_pooled_isa.py and tests/test_pooled_narrow_isa.py make of their units."""
import collections
import os
import re
import shutil
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, 'tools', 'perf'))

needs_hipcc = pytest.mark.skipif(
    not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')), reason='hipcc not available')


@pytest.fixture(scope='module')
def kernels():
    import isa
    return {name.replace('(anonymous namespace)::', ''): facts
            for name, facts in isa.kernel_table(source=isa.POOLED_KNOWN_SOURCE).items()}


@pytest.fixture(scope='module')
def assembly():
    import isa
    return isa.device_assembly(source=isa.POOLED_KNOWN_SOURCE)


def template_arguments(name):
    return name.split('<')[1].split('>')[0].split(', ')


@needs_hipcc
def test_the_known_pooled_kernel_families(kernels):
    # pool_known_trained: three key forms x (column form, pieces) x (fp32, bf16, fp16); the row-wise kernels per type
    families = collections.Counter(name.split('(')[0].split('<')[0].split(' ')[-1] for name in kernels)
    assert families == {'pool_known_trained': 18, 'pool_known_uniform': 3, 'pool_known_full': 3}, families
    forms = sorted(tuple(template_arguments(name)) for name in kernels if 'pool_known_trained<' in name)
    assert forms == sorted((has_sub, fast, vec4, out) for has_sub, fast in
                           (('false', 'true'), ('false', 'false'), ('true', 'false'))
                           for vec4 in ('false', 'true') for out in ('0', '1', '2')), forms
    for family in ('pool_known_uniform', 'pool_known_full'):
        assert sorted(template_arguments(name)[0] for name in kernels if family + '<' in name) == ['0', '1', '2']


@needs_hipcc
def test_known_pooled_kernels_spill_nothing_and_store_plainly(kernels, assembly):
    for name, facts in kernels.items():
        assert facts['private_segment'] == 0 and facts['scratch_ops'] == 0, (name, facts)
        assert facts['load_nt'] == 0 and facts['store_nt'] == 0, (name, facts)
    stores = re.findall(r'^\s*(?:global|flat|buffer)_store_\w+\s.*$', assembly, flags=re.M)
    assert stores and not [line for line in stores if re.search(r'\b(sc0|sc1|nt)\b', line)]
    # no atomics: the result is a function of the inputs alone
    assert not re.findall(r'^\s*(?:global|flat|buffer|ds)_atomic_\w+\s', assembly, flags=re.M)
    assert not re.findall(r'^\s*ds_\w+_rtn_\w+\s', assembly, flags=re.M)
    # the sums are single-lane v_add_f32: the packed forms flush subnormals on gfx950
    assert not re.findall(r'^\s*v_pk_(?:add|mul|fma)_f32\s', assembly, flags=re.M)
    assert len(re.findall(r'^\s*v_add_f32_e32\s', assembly, flags=re.M)) >= 24


@needs_hipcc
def test_known_trained_kernels_keep_the_one_tile_residency(kernels):
    # launchPooled plans them like pool_trained, with ONE_TILE_WAVES_PER_CU = 28: seven wavefronts per SIMD
    import isa
    for name, facts in kernels.items():
        if 'pool_known_trained<' in name:
            assert isa.waves_per_simd(facts['vgpr'], facts['sgpr_count']) == 7, (name, facts)
