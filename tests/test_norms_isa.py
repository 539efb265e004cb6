"""What the compiler made of memb_hip_norms.hip (tools/perf/isa.py, source=NORMS_SOURCE), without a GPU: no packed fp32
arithmetic, no scratch, the registers DESIGN.md section 5.7 states, a correctly rounded root and division -- and every
kernel of the units that existed before keeps the digest of the committed listing (profiles/norms_digests.txt)."""
import collections
import os
import re
import shutil
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, 'tools', 'perf'))

pytestmark = pytest.mark.skipif(
    not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')), reason='hipcc not available')

KEY_FORMS = (('false', 'true'), ('false', 'false'), ('true', 'false'))   # <HAS_SUB, FAST>
LISTING = os.path.join(REPO, 'profiles', 'norms_digests.txt')
# seven wavefronts per SIMD for the fused kernels (at most 64 vector registers, .sgpr_count at most
# 96), eight for the dense ones
TRAINED_VGPRS = 64
TRAINED_SGPRS = 96
NEW_KERNELS = ('norms_trained', 'unit_trained', 'norms_dense', 'unit_dense')


def kernel_family(name):
    return name.split('(')[0].split('<')[0].split(' ')[-1]


@pytest.fixture(scope='module')
def unit():
    import isa
    return {name.replace('(anonymous namespace)::', ''): facts
            for name, facts in isa.kernel_table(source=isa.NORMS_SOURCE).items()}


def test_the_unit_holds_the_fused_and_the_dense_kernels(unit):
    import isa
    assert collections.Counter(kernel_family(name) for name in unit) == {
        'norms_trained': 3, 'unit_trained': 3, 'norms_dense': 1, 'unit_dense': 1}
    for family in ('norms_trained', 'unit_trained'):
        forms = sorted(tuple(name.split('<')[1].split('>')[0].split(', ')) for name in unit if family + '<' in name)
        assert forms == sorted(KEY_FORMS)
    assert isa.NORMS_SOURCE in isa.SOURCES
    import build_native
    assert 'memb_hip_norms.hip' in open(build_native.__file__).read()


def test_no_packed_fp32_no_scratch_no_atomics(unit):
    for name, facts in unit.items():
        code = facts['code']
        assert not re.findall(r'^\s*v_pk_(?:add|mul|fma)_f32\s', code, flags=re.M), name
        assert facts['private_segment'] == 0 and facts['scratch_ops'] == 0, (name, facts['private_segment'])
        assert facts['load_nt'] == 0 and facts['store_nt'] == 0, name
        assert not re.findall(r'^\s*(?:global|flat|buffer|ds)_atomic_\w+\s', code, flags=re.M), name
        # the squares and the sums are single-lane instructions: 4 products and 3 adds per piece, 6 adds of the butterfly
        assert len(re.findall(r'^\s*v_mul_f32_e32\s', code, flags=re.M)) >= 4, name
        assert len(re.findall(r'^\s*v_add_f32_e32\s', code, flags=re.M)) >= 9, name
        # the butterfly: five exchanges within 32 lanes and one across the halves
        assert len(re.findall(r'^\s*ds_swizzle_b32\s', code, flags=re.M)) == 5, name
        assert len(re.findall(r'^\s*ds_bpermute_b32\s', code, flags=re.M)) >= 1, name


def test_registers_are_what_the_design_states(unit):
    import isa
    for name, facts in unit.items():
        if 'trained' in name:
            assert facts['vgpr'] <= TRAINED_VGPRS and facts['sgpr_count'] <= TRAINED_SGPRS, (name, facts['vgpr'], facts['sgpr_count'])
            assert isa.waves_per_simd(facts['vgpr'], facts['sgpr_count']) == 7, (name, facts['vgpr'], facts['sgpr_count'])
            assert facts['lds'] == 0, name   # (dynamic LDS only: the launch sizes it)
        else:
            assert isa.waves_per_simd(facts['vgpr'], facts['sgpr_count']) == 8, (name, facts['vgpr'], facts['sgpr_count'])


def test_norm_kernels_store_norms_only_and_unit_kernels_store_pieces(unit):
    for name, facts in unit.items():
        stores = collections.Counter(re.findall(r'^\s*(?:global|flat|buffer)_store_(\w+)\s', facts['code'], flags=re.M))
        if 'norms_' in name:
            assert set(stores) == {'dword'}, (name, stores)   # one float per row and no row
        elif 'unit_trained' in name:
            assert stores['dwordx4'] >= 2 and stores['dword'] >= 1, (name, stores)


def test_the_root_and_the_division_are_correctly_rounded(unit):
    # v_sqrt_f32 alone is one ulp: the library form steps to the neighbours and picks by the sign of two fused residuals;
    # the division is the scaled Newton iteration that ends in v_div_fmas_f32 / v_div_fixup_f32
    for name, facts in unit.items():
        code = facts['code']
        root = re.search(r'^\s*v_sqrt_f32\w*\s.*?(?=^\s*(?:global_store|s_endpgm|ds_))', code, flags=re.M | re.S)
        assert root, name
        assert len(re.findall(r'^\s*v_sqrt_f32', code, flags=re.M)) == 1, name
        assert len(re.findall(r'^\s*v_fma_f32\s+v\d+, -v\d+, v\d+, v\d+', root.group(0), flags=re.M)) >= 2, name
        assert not re.findall(r'^\s*v_rsq_f32', code, flags=re.M), name
        divisions = len(re.findall(r'^\s*v_div_fixup_f32\s', code, flags=re.M))
        assert divisions == len(re.findall(r'^\s*v_div_fmas_f32\s', code, flags=re.M)), name
        assert divisions == (8 if 'unit_trained' in name else 1 if 'unit_dense' in name else 0), (name, divisions)


def test_existing_units_keep_their_digests():
    import isa
    listed = {}
    for line in open(LISTING):
        fields = line.split()
        if fields:
            name = ' '.join(fields[:-5])
            listed[name] = tuple(fields[-5:])
    existing = [source for source in isa.SOURCES if source != isa.NORMS_SOURCE]
    assert len(existing) == 5
    now = {pretty.replace('(anonymous namespace)::', '').split('(')[0]: tuple(str(fact) for fact in facts)
           for pretty, facts in isa.kernel_digests(existing).items()}
    assert not [name for name in now if kernel_family(name) in NEW_KERNELS]
    changed = {name: (listed.get(name), facts) for name, facts in now.items() if listed.get(name) != facts}
    assert not changed, changed
    # and the listing holds nothing else but this unit's kernels
    extra = sorted(name for name in listed if name not in now and kernel_family(name) not in NEW_KERNELS)
    assert not extra, extra
