"""What the compiler made of memb_hip_queries.hip (tools/perf/isa.py, source=QUERIES_SOURCE), without a GPU: three
instances, no packed fp32 arithmetic, no scratch, no atomics, the registers DESIGN.md section 5.10 states, two correctly
rounded roots, the cosine's one division, three butterflies, one to three 4-byte stores -- and every kernel of the units
that existed before keeps the digest of its committed listing (profiles/norms_digests.txt, profiles/pairs_digests.txt,
profiles/bag_pairs_digests.txt), which are themselves what they were."""
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
NORMS_LISTING = os.path.join(REPO, 'profiles', 'norms_digests.txt')
NORMS_LISTING_SHA256 = '3c7796ca9b542e388633d0113a19c6f0f47ba5d9221263d089c85da38d6fb5d2'   # as tests/test_pairs_isa.py has it
PAIRS_LISTING = os.path.join(REPO, 'profiles', 'pairs_digests.txt')
PAIRS_LISTING_SHA256 = '565e6a7a9a4f5a94fd7c69f049d90b1220077c941a764711a30a55ad6675fe38'   # as tests/test_bag_pairs_isa.py has it
BAG_PAIRS_LISTING = os.path.join(REPO, 'profiles', 'bag_pairs_digests.txt')   # tools/perf/isa.py --digests <BAG_PAIRS_SOURCE> of the parent commit
BAG_PAIRS_LISTING_SHA256 = '549b2e3170342c56764b032fba795781c805c633fdc7246e09ed028324622c2a'
# seven wavefronts per SIMD (at most 72 vector registers, .sgpr_count at most 96)
TRAINED_WAVES = 7
SGPR_COUNT = 94


def kernel_family(name):
    return name.split('(')[0].split('<')[0].split(' ')[-1]


def count(code, pattern):
    return len(re.findall(r'^\s*' + pattern, code, flags=re.M))


@pytest.fixture(scope='module')
def unit():
    import isa
    return {name.replace('(anonymous namespace)::', ''): facts
            for name, facts in isa.kernel_table(source=isa.QUERIES_SOURCE).items()}


def test_the_unit_holds_three_instances(unit):
    import isa
    assert collections.Counter(kernel_family(name) for name in unit) == {'query_trained': 3}
    forms = sorted(tuple(name.split('<')[1].split('>')[0].split(', ')) for name in unit)
    assert forms == sorted(KEY_FORMS)
    # a unit of its own, beside the eight of LIBRARY_SOURCES
    assert isa.QUERIES_SOURCE not in isa.LIBRARY_SOURCES and len(isa.LIBRARY_SOURCES) == 8
    assert isa.EVERY_SOURCE == isa.LIBRARY_SOURCES + (isa.QUERIES_SOURCE,)
    import build_native
    assert 'memb_hip_queries.hip' in open(build_native.__file__).read()


def test_no_packed_fp32_no_scratch_no_atomics(unit):
    for name, facts in unit.items():
        code = facts['code']
        assert not count(code, r'v_pk_(?:add|mul|fma)_f32\s'), name
        assert facts['private_segment'] == 0 and facts['scratch_ops'] == 0, (name, facts['private_segment'])
        assert not count(code, r'(?:global|flat|buffer|ds)_atomic_\w+\s'), name


def test_three_butterflies_side_by_side(unit):
    for name, facts in unit.items():
        assert count(facts['code'], r'ds_swizzle_b32\s') == 15, name


def test_registers_are_what_the_design_states(unit):
    import isa
    design = open(os.path.join(REPO, 'DESIGN.md')).read()
    section = design[design.index('### 5.10'):]
    assert '| `query_trained<HAS_SUB, FAST>` (3) |' in section
    assert '| {} | {} | `pool_trained`'.format(SGPR_COUNT, TRAINED_WAVES) in section   # the table's .sgpr_count and waves / SIMD columns
    for name, facts in unit.items():
        assert facts['sgpr_count'] == SGPR_COUNT, (name, facts['sgpr_count'])
        assert isa.waves_per_simd(facts['vgpr'], facts['sgpr_count']) == TRAINED_WAVES, (name, facts['vgpr'], facts['sgpr_count'])
        assert facts['lds'] == 0, name   # (dynamic LDS only: the launch sizes it)
    # what the launch plans its grid for
    header = open(os.path.join(REPO, 'memb_amd', 'csrc', 'hip_queries.h')).read()
    assert 'TRAINED_WAVES_PER_SIMD = {};'.format(TRAINED_WAVES) in header


def test_no_row_is_stored(unit):
    for name, facts in unit.items():
        stores = collections.Counter(re.findall(r'^\s*(?:global|flat|buffer)_store_(\w+)\s', facts['code'], flags=re.M))
        assert set(stores) == {'dword'}, (name, stores)
        assert 1 <= stores['dword'] <= 3, (name, stores)   # the cosine, the dot, the norm


def test_the_roots_and_the_division_are_correctly_rounded(unit):
    # v_sqrt_f32 alone is one ulp: the library form steps to the neighbours and picks by the sign of two fused residuals;
    # a division is the scaled Newton iteration that ends in v_div_fmas_f32 / v_div_fixup_f32
    for name, facts in unit.items():
        code = facts['code']
        roots = [(match.start(), match.group(1)) for match in re.finditer(r'^\s*v_sqrt_f32\w*\s+(v\d+), v\d+', code, flags=re.M)]
        assert len(roots) == 2 and count(code, r'v_sqrt_f32') == 2, (name, roots)
        # up to the cosine's division, each root's register is the factor of two residuals of its own (the two roots may be
        # scheduled into each other, or one after the other in the same register)
        end = re.compile(r'^\s*(?:v_div_scale_f32|global_store|s_endpgm)', flags=re.M).search(code, roots[-1][0]).start()
        for register in {register for _, register in roots}:
            residuals = re.findall(r'^\s*v_fma_f32\s+v\d+, -v\d+, ' + register + r', v\d+', code[roots[0][0]:end], flags=re.M)
            assert len(residuals) >= 2 * sum(1 for _, other in roots if other == register), (name, register, residuals)
        assert not count(code, r'v_rsq_f32'), name
        assert count(code, r'v_div_fixup_f32\s') == 1 and count(code, r'v_div_fmas_f32\s') == 1, name


def listed_digests(path):
    listed = {}
    for line in open(path):
        fields = line.split()
        if fields:
            listed[' '.join(fields[:-5])] = tuple(fields[-5:])
    return listed


def digests_now(sources):
    import isa
    return {pretty.replace('(anonymous namespace)::', '').split('(')[0]: tuple(str(fact) for fact in facts)
            for pretty, facts in isa.kernel_digests(sources).items()}


def kept(listing, sha256, sources, kernels=None):
    assert hashlib.sha256(open(listing, 'rb').read()).hexdigest() == sha256
    listed, now = listed_digests(listing), digests_now(sources)
    assert kernels is None or len(listed) == kernels
    changed = {name: (listed.get(name), facts) for name, facts in now.items() if listed.get(name) != facts}
    assert not changed, changed
    assert sorted(listed) == sorted(now)


def test_the_six_units_keep_their_digests():
    import isa
    kept(NORMS_LISTING, NORMS_LISTING_SHA256, isa.SOURCES)


def test_the_pairs_unit_keeps_its_digests():
    import isa
    kept(PAIRS_LISTING, PAIRS_LISTING_SHA256, (isa.PAIRS_SOURCE,), kernels=4)


def test_the_bag_pairs_unit_keeps_its_digests():
    import isa
    kept(BAG_PAIRS_LISTING, BAG_PAIRS_LISTING_SHA256, (isa.BAG_PAIRS_SOURCE,), kernels=3)
