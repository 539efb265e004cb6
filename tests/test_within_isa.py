"""What the compiler made of memb_hip_within.hip (tools/perf/isa.py, source=WITHIN_SOURCE), without a GPU: three kernels,
no scratch, the registers, LDS and wavefronts per SIMD DESIGN.md section 5.17 states -- and every kernel of the units that
existed before keeps the digest of its committed listing (profiles/ranks_digests.txt, taken at the parent commit, and the
older listings)."""
import os
import shutil
import sys

import pytest

from conftest import REPO
from test_analogies_isa import QUERY_BAGS_LISTING
from test_cosmul_isa import ANALOGIES_LISTING
from test_query_bags_isa import QUERY_TOPK_LISTING
from test_query_matrix_isa import QUERIES_LISTING, kept
from test_query_topk_isa import QUERY_MATRIX_LISTING
from test_ranks_isa import COSMUL_LISTING

sys.path.insert(0, os.path.join(REPO, 'tools', 'perf'))

pytestmark = pytest.mark.skipif(
    not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')), reason='hipcc not available')

RANKS_LISTING = os.path.join(REPO, 'profiles', 'ranks_digests.txt')   # tools/perf/isa.py --digests <RANKS_SOURCE> of the parent commit
# eight wavefronts per SIMD (at most 64 vector registers, .sgpr_count at most 80)
WAVES = 8
REGISTERS = {'within_count': (51, 54, 288), 'within_starts': (23, 28, 0), 'within_write': (51, 66, 400)}   # (vector registers, .sgpr_count, bytes of LDS)


@pytest.fixture(scope='module')
def unit():
    import isa
    return {name.replace('(anonymous namespace)::', '').split('(')[0]: facts
            for name, facts in isa.kernel_table(source=isa.WITHIN_SOURCE).items()}


def test_the_unit_holds_three_kernels(unit):
    import isa
    assert sorted(unit) == ['within_count', 'within_starts', 'within_write']
    # a unit of its own, beside the fifteen of WITH_RANKS
    assert isa.WITHIN_SOURCE not in isa.WITH_RANKS and len(isa.WITH_RANKS) == 15
    assert isa.WITH_WITHIN == isa.WITH_RANKS + (isa.WITHIN_SOURCE,)
    import build_native
    assert 'memb_hip_within.hip' in open(build_native.__file__).read()


def test_no_scratch(unit):
    for name, facts in unit.items():
        assert facts['private_segment'] == 0 and facts['scratch_ops'] == 0, name


def test_registers_are_what_the_design_states(unit):
    import isa
    design = open(os.path.join(REPO, 'DESIGN.md')).read()
    section = design[design.index('### 5.17'):]
    for name, (vgpr, sgpr_count, lds) in REGISTERS.items():
        facts = unit[name]
        assert (facts['vgpr'], facts['sgpr_count'], facts['lds']) == (vgpr, sgpr_count, lds), (name, facts['vgpr'], facts['sgpr_count'], facts['lds'])
        assert isa.waves_per_simd(facts['vgpr'], facts['sgpr_count']) == WAVES, name
        assert '| `{}` | {} | {} | {} | {} |'.format(name, vgpr, sgpr_count, WAVES, lds) in section, name   # the table's register columns


def test_the_rank_unit_keeps_its_digests():
    import isa
    kept(RANKS_LISTING, (isa.RANKS_SOURCE,), kernels=2)


def test_the_older_units_keep_their_digests():
    import isa
    kept(COSMUL_LISTING, (isa.COSMUL_SOURCE,), kernels=1)
    kept(ANALOGIES_LISTING, (isa.ANALOGIES_SOURCE,), kernels=2)
    kept(QUERY_BAGS_LISTING, (isa.QUERY_BAGS_SOURCE,), kernels=3)
    kept(QUERY_TOPK_LISTING, (isa.QUERY_TOPK_SOURCE,), kernels=2)
    kept(QUERY_MATRIX_LISTING, (isa.QUERY_MATRIX_SOURCE,), kernels=3)
    kept(QUERIES_LISTING, (isa.QUERIES_SOURCE,), kernels=3)
    kept(os.path.join(REPO, 'profiles', 'norms_digests.txt'), isa.SOURCES)
    kept(os.path.join(REPO, 'profiles', 'pairs_digests.txt'), (isa.PAIRS_SOURCE,), kernels=4)
    kept(os.path.join(REPO, 'profiles', 'bag_pairs_digests.txt'), (isa.BAG_PAIRS_SOURCE,), kernels=3)
