"""What the compiler made of memb_hip_query_bags.hip (tools/perf/isa.py, source=QUERY_BAGS_SOURCE), without a GPU: three
kernels, no scratch, no atomics, the registers and wavefronts per SIMD DESIGN.md section 5.13 states -- and every kernel of
the units that existed before keeps the digest of its committed listing (profiles/query_topk_digests.txt, taken at the
parent commit, and the older listings)."""
import os
import re
import shutil
import sys

import pytest

from conftest import REPO
from test_query_matrix_isa import QUERIES_LISTING, kept
from test_query_topk_isa import QUERY_MATRIX_LISTING

sys.path.insert(0, os.path.join(REPO, 'tools', 'perf'))

pytestmark = pytest.mark.skipif(
    not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')), reason='hipcc not available')

QUERY_TOPK_LISTING = os.path.join(REPO, 'profiles', 'query_topk_digests.txt')   # tools/perf/isa.py --digests <QUERY_TOPK_SOURCE> of the parent commit
# five wavefronts per SIMD (at most 96 vector registers)
WAVES = 5
REGISTERS = {'query_bags_trained<false, true>': (81, 94), 'query_bags_trained<false, false>': (82, 94),
             'query_bags_trained<true, false>': (83, 94)}   # (vector registers, .sgpr_count)


@pytest.fixture(scope='module')
def unit():
    import isa
    return {name.replace('(anonymous namespace)::', '').split('(')[0].replace('void ', ''): facts
            for name, facts in isa.kernel_table(source=isa.QUERY_BAGS_SOURCE).items()}


def test_the_unit_holds_the_three_key_forms(unit):
    import isa
    assert sorted(unit) == sorted(REGISTERS)
    # a unit of its own, beside the eleven of WITH_QUERY_TOPK
    assert isa.QUERY_BAGS_SOURCE not in isa.WITH_QUERY_TOPK and len(isa.WITH_QUERY_TOPK) == 11
    assert isa.WITH_QUERY_BAGS == isa.WITH_QUERY_TOPK + (isa.QUERY_BAGS_SOURCE,)
    import build_native
    assert 'memb_hip_query_bags.hip' in open(build_native.__file__).read()


def test_no_scratch_no_atomics(unit):
    for name, facts in unit.items():
        assert facts['private_segment'] == 0 and facts['scratch_ops'] == 0, (name, facts['private_segment'])
        assert not re.search(r'^\s*(?:global|flat|buffer|ds)_atomic', facts['code'], flags=re.M), name
        # no row is stored: the results leave as single floats, lane by lane
        assert set(re.findall(r'^\s*global_store_(\w+)\s', facts['code'], flags=re.M)) == {'dword'}, name
        assert not re.search(r'^\s*v_(?:mfma|pk_(?:mul|add|fma)_f32)', facts['code'], flags=re.M), name


def test_registers_are_what_the_design_states(unit):
    import isa
    design = open(os.path.join(REPO, 'DESIGN.md')).read()
    section = design[design.index('### 5.13'):]
    for name, (vgpr, sgpr_count) in REGISTERS.items():
        facts = unit[name]
        assert (facts['vgpr'], facts['sgpr_count']) == (vgpr, sgpr_count), (name, facts['vgpr'], facts['sgpr_count'])
        assert isa.waves_per_simd(facts['vgpr'], facts['sgpr_count']) == WAVES, name
        assert '| `{}` | {} | {} | {} | 0 |'.format(name, vgpr, sgpr_count, WAVES) in section, name   # the table's register columns


def test_the_query_topk_unit_keeps_its_digests():
    import isa
    kept(QUERY_TOPK_LISTING, (isa.QUERY_TOPK_SOURCE,), kernels=2)


def test_the_older_units_keep_their_digests():
    import isa
    kept(QUERY_MATRIX_LISTING, (isa.QUERY_MATRIX_SOURCE,), kernels=3)
    kept(QUERIES_LISTING, (isa.QUERIES_SOURCE,), kernels=3)
    kept(os.path.join(REPO, 'profiles', 'norms_digests.txt'), isa.SOURCES)
    kept(os.path.join(REPO, 'profiles', 'pairs_digests.txt'), (isa.PAIRS_SOURCE,), kernels=4)
    kept(os.path.join(REPO, 'profiles', 'bag_pairs_digests.txt'), (isa.BAG_PAIRS_SOURCE,), kernels=3)
