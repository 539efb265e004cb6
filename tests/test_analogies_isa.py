"""What the compiler made of memb_hip_analogies.hip (tools/perf/isa.py, source=ANALOGIES_SOURCE), without a GPU: two
kernels, no scratch, no LDS, no atomics, the registers and wavefronts per SIMD DESIGN.md section 5.14 states, no fused
multiply-add in the weighted sum -- and every kernel of the units that existed before keeps the digest of its committed
listing (profiles/query_bags_digests.txt, taken at the parent commit, and the older listings): sharing
hip_query_topk_kernels.h with the new unit changes no instruction of topk_select or topk_merge."""
import os
import re
import shutil
import sys

import pytest

from conftest import REPO
from test_query_bags_isa import QUERY_TOPK_LISTING
from test_query_matrix_isa import QUERIES_LISTING, kept
from test_query_topk_isa import QUERY_MATRIX_LISTING

sys.path.insert(0, os.path.join(REPO, 'tools', 'perf'))

pytestmark = pytest.mark.skipif(
    not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')), reason='hipcc not available')

QUERY_BAGS_LISTING = os.path.join(REPO, 'profiles', 'query_bags_digests.txt')   # tools/perf/isa.py --digests <QUERY_BAGS_SOURCE> of the parent commit
# eight wavefronts per SIMD (at most 64 vector registers, .sgpr_count at most 80)
WAVES = 8
REGISTERS = {'topk_select_excluding': (29, 42), 'weighted_rows_sum': (14, 29)}   # (vector registers, .sgpr_count)


@pytest.fixture(scope='module')
def unit():
    import isa
    return {name.replace('(anonymous namespace)::', '').split('(')[0]: facts
            for name, facts in isa.kernel_table(source=isa.ANALOGIES_SOURCE).items()}


def test_the_unit_holds_two_kernels(unit):
    import isa
    assert sorted(unit) == ['topk_select_excluding', 'weighted_rows_sum']
    # a unit of its own, beside the twelve of WITH_QUERY_BAGS
    assert isa.ANALOGIES_SOURCE not in isa.WITH_QUERY_BAGS and len(isa.WITH_QUERY_BAGS) == 12
    assert isa.WITH_ANALOGIES == isa.WITH_QUERY_BAGS + (isa.ANALOGIES_SOURCE,)
    import build_native
    assert 'memb_hip_analogies.hip' in open(build_native.__file__).read()


def test_no_scratch_no_lds_no_atomics(unit):
    for name, facts in unit.items():
        assert facts['private_segment'] == 0 and facts['scratch_ops'] == 0, (name, facts['private_segment'])
        assert facts['lds'] == 0 and not re.search(r'^\s*ds_(?:read|write)', facts['code'], flags=re.M), name
        assert not re.search(r'^\s*(?:global|flat|buffer)_atomic', facts['code'], flags=re.M), name
        # the selection writes its lists, the sum single floats: 4-byte stores only
        assert set(re.findall(r'^\s*global_store_(\w+)\s', facts['code'], flags=re.M)) == {'dword'}, name
    # two rounded operations: a multiply and an add, never a fused multiply-add
    code = unit['weighted_rows_sum']['code']
    assert re.search(r'^\s*v_mul_f32', code, flags=re.M) and re.search(r'^\s*v_add_f32', code, flags=re.M)
    assert not re.search(r'^\s*v_(?:pk_)?(?:fma|fmac|mad|mac)_(?:legacy_)?f\d+', code, flags=re.M)   # (v_mad_u64_u32 is an address)


def test_registers_are_what_the_design_states(unit):
    import isa
    design = open(os.path.join(REPO, 'DESIGN.md')).read()
    section = design[design.index('### 5.14'):]
    for name, (vgpr, sgpr_count) in REGISTERS.items():
        facts = unit[name]
        assert (facts['vgpr'], facts['sgpr_count']) == (vgpr, sgpr_count), (name, facts['vgpr'], facts['sgpr_count'])
        assert isa.waves_per_simd(facts['vgpr'], facts['sgpr_count']) == WAVES, name
        assert '| `{}` | {} | {} | {} | 0 |'.format(name, vgpr, sgpr_count, WAVES) in section, name   # the table's register columns


def test_the_query_bags_unit_keeps_its_digests():
    import isa
    kept(QUERY_BAGS_LISTING, (isa.QUERY_BAGS_SOURCE,), kernels=3)


def test_the_older_units_keep_their_digests():
    import isa
    kept(QUERY_TOPK_LISTING, (isa.QUERY_TOPK_SOURCE,), kernels=2)
    kept(QUERY_MATRIX_LISTING, (isa.QUERY_MATRIX_SOURCE,), kernels=3)
    kept(QUERIES_LISTING, (isa.QUERIES_SOURCE,), kernels=3)
    kept(os.path.join(REPO, 'profiles', 'norms_digests.txt'), isa.SOURCES)
    kept(os.path.join(REPO, 'profiles', 'pairs_digests.txt'), (isa.PAIRS_SOURCE,), kernels=4)
    kept(os.path.join(REPO, 'profiles', 'bag_pairs_digests.txt'), (isa.BAG_PAIRS_SOURCE,), kernels=3)
