"""What the compiler made of memb_hip_query_matrix.hip (tools/perf/isa.py, source=QUERY_MATRIX_SOURCE), without a GPU:
three instances, no scratch, no packed fp32 arithmetic, only 4-byte global stores, the registers and wavefronts per SIMD
DESIGN.md section 5.11 states -- and every kernel of the units that existed before keeps the digest of its committed
listing (profiles/queries_digests.txt, taken at the parent commit, and the three older listings)."""
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
QUERIES_LISTING = os.path.join(REPO, 'profiles', 'queries_digests.txt')   # tools/perf/isa.py --digests <QUERIES_SOURCE> of the parent commit
# seven wavefronts per SIMD (at most 72 vector registers, .sgpr_count at most 96)
TRAINED_WAVES = 7
SGPR_COUNT = 94
VGPRS = (70, 71)


def kernel_family(name):
    return name.split('(')[0].split('<')[0].split(' ')[-1]


def count(code, pattern):
    return len(re.findall(r'^\s*' + pattern, code, flags=re.M))


@pytest.fixture(scope='module')
def unit():
    import isa
    return {name.replace('(anonymous namespace)::', ''): facts
            for name, facts in isa.kernel_table(source=isa.QUERY_MATRIX_SOURCE).items()}


def test_the_unit_holds_three_instances(unit):
    import isa
    assert collections.Counter(kernel_family(name) for name in unit) == {'query_matrix_trained': 3}
    forms = sorted(tuple(name.split('<')[1].split('>')[0].split(', ')) for name in unit)
    assert forms == sorted(KEY_FORMS)
    # a unit of its own, beside the nine of EVERY_SOURCE
    assert isa.QUERY_MATRIX_SOURCE not in isa.EVERY_SOURCE and len(isa.EVERY_SOURCE) == 9
    assert isa.WHOLE_LIBRARY == isa.EVERY_SOURCE + (isa.QUERY_MATRIX_SOURCE,)
    import build_native
    assert 'memb_hip_query_matrix.hip' in open(build_native.__file__).read()


def test_no_scratch_and_no_packed_fp32(unit):
    for name, facts in unit.items():
        assert facts['private_segment'] == 0 and facts['scratch_ops'] == 0, (name, facts['private_segment'])
        assert not count(facts['code'], r'v_pk_(?:add|mul|fma)_f32\s'), name


def test_only_four_byte_global_stores(unit):
    for name, facts in unit.items():
        stores = collections.Counter(re.findall(r'^\s*(?:global|flat|buffer)_store_(\w+)\s', facts['code'], flags=re.M))
        assert set(stores) == {'dword'}, (name, stores)


def test_registers_are_what_the_design_states(unit):
    import isa
    design = open(os.path.join(REPO, 'DESIGN.md')).read()
    section = design[design.index('### 5.11'):]
    assert '| `query_matrix_trained<HAS_SUB, FAST>` (3) |' in section
    assert '| {}-{} | {} | {} | `pool_trained`'.format(VGPRS[0], VGPRS[1], SGPR_COUNT, TRAINED_WAVES) in section   # the table's register columns
    for name, facts in unit.items():
        assert VGPRS[0] <= facts['vgpr'] <= VGPRS[1], (name, facts['vgpr'])
        assert facts['sgpr_count'] == SGPR_COUNT, (name, facts['sgpr_count'])
        assert isa.waves_per_simd(facts['vgpr'], facts['sgpr_count']) == TRAINED_WAVES, (name, facts['vgpr'], facts['sgpr_count'])
        assert facts['lds'] == 0, name   # (dynamic LDS only: the launch sizes it)
    # what the launch plans its grid for, and the block of queries the table states
    header = open(os.path.join(REPO, 'memb_amd', 'csrc', 'hip_query_matrix.h')).read()
    assert 'TRAINED_WAVES_PER_SIMD = {};'.format(TRAINED_WAVES) in header and 'QUERY_BLOCK = 2;' in header


def listed_digests(path):
    listed = {}
    for line in open(path):
        fields = line.split()
        if fields:
            listed[' '.join(fields[:-5])] = tuple(fields[-5:])
    return listed


def kept(listing, sources, kernels=None):
    import isa
    listed = listed_digests(listing)
    now = {pretty.replace('(anonymous namespace)::', '').split('(')[0]: tuple(str(fact) for fact in facts)
           for pretty, facts in isa.kernel_digests(sources).items()}
    assert kernels is None or len(listed) == kernels
    changed = {name: (listed.get(name), facts) for name, facts in now.items() if listed.get(name) != facts}
    assert not changed, changed
    assert sorted(listed) == sorted(now)


def test_the_queries_unit_keeps_its_digests():
    import isa
    kept(QUERIES_LISTING, (isa.QUERIES_SOURCE,), kernels=3)


def test_the_older_units_keep_their_digests():
    import isa
    kept(os.path.join(REPO, 'profiles', 'norms_digests.txt'), isa.SOURCES)
    kept(os.path.join(REPO, 'profiles', 'pairs_digests.txt'), (isa.PAIRS_SOURCE,), kernels=4)
    kept(os.path.join(REPO, 'profiles', 'bag_pairs_digests.txt'), (isa.BAG_PAIRS_SOURCE,), kernels=3)
