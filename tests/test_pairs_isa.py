"""What the compiler made of memb_hip_pairs.hip (tools/perf/isa.py, source=PAIRS_SOURCE), without a GPU: no packed fp32
arithmetic, no scratch, the registers DESIGN.md section 5.8 states, two correctly rounded roots and one correctly rounded
division per kernel, three butterflies, 4-byte stores only -- and every kernel of the six units that existed before keeps
the digest of the committed listing (profiles/norms_digests.txt), which is itself what it was."""
import collections
import hashlib
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
LISTING_SHA256 = '3c7796ca9b542e388633d0113a19c6f0f47ba5d9221263d089c85da38d6fb5d2'
# seven wavefronts per SIMD for the fused kernel (at most 64 vector registers, .sgpr_count at most
# 96), eight for the dense one
TRAINED_WAVES = 7
DENSE_WAVES = 8


def kernel_family(name):
    return name.split('(')[0].split('<')[0].split(' ')[-1]


def count(code, pattern):
    return len(re.findall(r'^\s*' + pattern, code, flags=re.M))


@pytest.fixture(scope='module')
def unit():
    import isa
    return {name.replace('(anonymous namespace)::', ''): facts
            for name, facts in isa.kernel_table(source=isa.PAIRS_SOURCE).items()}


def test_the_unit_holds_the_fused_and_the_dense_kernel(unit):
    import isa
    assert collections.Counter(kernel_family(name) for name in unit) == {'pairs_trained': 3, 'pairs_dense': 1}
    forms = sorted(tuple(name.split('<')[1].split('>')[0].split(', ')) for name in unit if 'pairs_trained<' in name)
    assert forms == sorted(KEY_FORMS)
    # a unit of its own, beside the six that tests/test_norms_isa.py counts
    assert isa.PAIRS_SOURCE not in isa.SOURCES and len(isa.SOURCES) == 6
    assert isa.ALL_SOURCES == isa.SOURCES + (isa.PAIRS_SOURCE,)
    import build_native
    assert 'memb_hip_pairs.hip' in open(build_native.__file__).read()


def test_no_packed_fp32_no_scratch_no_atomics(unit):
    for name, facts in unit.items():
        code = facts['code']
        assert not count(code, r'v_pk_(?:add|mul|fma)_f32\s'), name
        assert facts['private_segment'] == 0 and facts['scratch_ops'] == 0, (name, facts['private_segment'])
        assert facts['load_nt'] == 0 and facts['store_nt'] == 0, name
        assert not count(code, r'(?:global|flat|buffer|ds)_atomic_\w+\s'), name
        # 12 products and 9 sums per piece of a pair, 18 sums of the three butterflies: single-lane instructions
        assert count(code, r'v_mul_f32_e32\s') >= 12, name
        assert count(code, r'v_add_f32_e32\s') >= 27, name


def test_three_butterflies_side_by_side(unit):
    for name, facts in unit.items():
        code = facts['code']
        assert count(code, r'ds_swizzle_b32\s') == 15, name
        assert count(code, r'ds_bpermute_b32\s') >= 3, name
        # per stride the three exchanges are all issued in front of the first of the three sums
        lines = [line.strip() for line in code.split('\n')]
        swizzles = [i for i, line in enumerate(lines) if line.startswith('ds_swizzle_b32')]
        for first, last in zip(swizzles[0::3], swizzles[2::3]):
            assert not [line for line in lines[first:last] if line.startswith('v_add_f32')], (name, lines[first:last + 1])
            assert len({line.split('offset:')[1] for line in lines[first:last + 1] if line.startswith('ds_swizzle')}) == 1, name


def test_registers_are_what_the_design_states(unit):
    import isa
    design = open(os.path.join(REPO, 'DESIGN.md')).read()
    section = design[design.index('### 5.8'):]
    assert '| {} | `pool_trained`'.format(TRAINED_WAVES) in section   # the table's waves / SIMD column of pairs_trained
    for name, facts in unit.items():
        waves = isa.waves_per_simd(facts['vgpr'], facts['sgpr_count'])
        if 'trained' in name:
            assert waves == TRAINED_WAVES, (name, facts['vgpr'], facts['sgpr_count'])
            assert facts['lds'] == 0, name   # (dynamic LDS only: the launch sizes it)
        else:
            assert waves == DENSE_WAVES, (name, facts['vgpr'], facts['sgpr_count'])


def test_no_row_is_stored(unit):
    for name, facts in unit.items():
        stores = collections.Counter(re.findall(r'^\s*(?:global|flat|buffer)_store_(\w+)\s', facts['code'], flags=re.M))
        assert set(stores) == {'dword'}, (name, stores)
        assert 1 <= stores['dword'] <= 3, (name, stores)   # the cosines, the dots, the norms: one store each at most


def test_the_roots_and_the_division_are_correctly_rounded(unit):
    # v_sqrt_f32 alone is one ulp: the library form steps to the neighbours and picks by the sign of two fused residuals;
    # the division is the scaled Newton iteration that ends in v_div_fmas_f32 / v_div_fixup_f32
    for name, facts in unit.items():
        code = facts['code']
        roots = re.findall(r'^\s*v_sqrt_f32\w*\s+(v\d+), v\d+', code, flags=re.M)
        assert len(roots) == 2 and count(code, r'v_sqrt_f32') == 2 and roots[0] != roots[1], (name, roots)
        # (the two roots are scheduled into each other: up to the division, each root's register is the factor of two residuals)
        tail = re.search(r'^\s*v_sqrt_f32.*?(?=^\s*(?:v_div_scale_f32|global_store|s_endpgm))', code, flags=re.M | re.S)
        assert tail, name
        for root in roots:
            residuals = re.findall(r'^\s*v_fma_f32\s+v\d+, -v\d+, ' + root + r', v\d+', tail.group(0), flags=re.M)
            assert len(residuals) >= 2, (name, root, residuals)
        assert not count(code, r'v_rsq_f32'), name
        assert count(code, r'v_div_fixup_f32\s') == 1 and count(code, r'v_div_fmas_f32\s') == 1, name


def test_existing_units_keep_their_digests():
    import isa
    # the listing is the committed one
    assert hashlib.sha256(open(LISTING, 'rb').read()).hexdigest() == LISTING_SHA256
    listed = {}
    for line in open(LISTING):
        fields = line.split()
        if fields:
            listed[' '.join(fields[:-5])] = tuple(fields[-5:])
    now = {pretty.replace('(anonymous namespace)::', '').split('(')[0]: tuple(str(fact) for fact in facts)
           for pretty, facts in isa.kernel_digests(isa.SOURCES).items()}
    assert not [name for name in now if kernel_family(name).startswith('pairs_')]
    changed = {name: (listed.get(name), facts) for name, facts in now.items() if listed.get(name) != facts}
    assert not changed, changed
    assert sorted(listed) == sorted(now)
