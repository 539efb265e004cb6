"""What the compiler made of memb_hip_query_topk.hip (tools/perf/isa.py, source=QUERY_TOPK_SOURCE), without a GPU: two
kernels, no scratch, no LDS, no atomics, the registers and wavefronts per SIMD DESIGN.md section 5.12 states -- and every
kernel of the units that existed before keeps the digest of its committed listing (profiles/query_matrix_digests.txt, taken
at the parent commit, and the four older listings)."""
import os
import re
import shutil
import sys

import pytest

from conftest import REPO
from test_query_matrix_isa import QUERIES_LISTING, kept

sys.path.insert(0, os.path.join(REPO, 'tools', 'perf'))

pytestmark = pytest.mark.skipif(
    not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')), reason='hipcc not available')

QUERY_MATRIX_LISTING = os.path.join(REPO, 'profiles', 'query_matrix_digests.txt')   # tools/perf/isa.py --digests <QUERY_MATRIX_SOURCE> of the parent commit
# eight wavefronts per SIMD (at most 64 vector registers, .sgpr_count at most 80)
WAVES = 8
REGISTERS = {'topk_select': (28, 38), 'topk_merge': (27, 29)}   # (vector registers, .sgpr_count)


@pytest.fixture(scope='module')
def unit():
    import isa
    return {name.replace('(anonymous namespace)::', '').split('(')[0]: facts
            for name, facts in isa.kernel_table(source=isa.QUERY_TOPK_SOURCE).items()}


def test_the_unit_holds_two_kernels(unit):
    import isa
    assert sorted(unit) == ['topk_merge', 'topk_select']
    # a unit of its own, beside the ten of WHOLE_LIBRARY
    assert isa.QUERY_TOPK_SOURCE not in isa.WHOLE_LIBRARY and len(isa.WHOLE_LIBRARY) == 10
    assert isa.WITH_QUERY_TOPK == isa.WHOLE_LIBRARY + (isa.QUERY_TOPK_SOURCE,)
    import build_native
    assert 'memb_hip_query_topk.hip' in open(build_native.__file__).read()


def test_no_scratch_no_lds_no_atomics(unit):
    for name, facts in unit.items():
        assert facts['private_segment'] == 0 and facts['scratch_ops'] == 0, (name, facts['private_segment'])
        assert facts['lds'] == 0 and not re.search(r'^\s*ds_(?:read|write)', facts['code'], flags=re.M), name
        assert not re.search(r'^\s*(?:global|flat|buffer)_atomic', facts['code'], flags=re.M), name
    # the selection writes its lists only, the merge the two outputs: 4-byte and 8-byte stores
    assert set(re.findall(r'^\s*global_store_(\w+)\s', unit['topk_select']['code'], flags=re.M)) == {'dword'}
    assert set(re.findall(r'^\s*global_store_(\w+)\s', unit['topk_merge']['code'], flags=re.M)) == {'dword', 'dwordx2'}


def test_registers_are_what_the_design_states(unit):
    import isa
    design = open(os.path.join(REPO, 'DESIGN.md')).read()
    section = design[design.index('### 5.12'):]
    for name, (vgpr, sgpr_count) in REGISTERS.items():
        facts = unit[name]
        assert (facts['vgpr'], facts['sgpr_count']) == (vgpr, sgpr_count), (name, facts['vgpr'], facts['sgpr_count'])
        assert isa.waves_per_simd(facts['vgpr'], facts['sgpr_count']) == WAVES, name
        assert '| `{}` | {} | {} | {} | 0 |'.format(name, vgpr, sgpr_count, WAVES) in section, name   # the table's register columns


def test_the_query_matrix_unit_keeps_its_digests():
    import isa
    kept(QUERY_MATRIX_LISTING, (isa.QUERY_MATRIX_SOURCE,), kernels=3)


def test_the_older_units_keep_their_digests():
    import isa
    kept(QUERIES_LISTING, (isa.QUERIES_SOURCE,), kernels=3)
    kept(os.path.join(REPO, 'profiles', 'norms_digests.txt'), isa.SOURCES)
    kept(os.path.join(REPO, 'profiles', 'pairs_digests.txt'), (isa.PAIRS_SOURCE,), kernels=4)
    kept(os.path.join(REPO, 'profiles', 'bag_pairs_digests.txt'), (isa.BAG_PAIRS_SOURCE,), kernels=3)
