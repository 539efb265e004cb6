"""What the compiler made of memb_hip_ranks.hip (tools/perf/isa.py, source=RANKS_SOURCE), without a GPU: two kernels, no
scratch, no atomics, rank_count's loads back to back with no wait or branch between them and one store of a partial count,
the registers and wavefronts per SIMD DESIGN.md section 5.16 states -- and every kernel of the units that existed before
keeps the digest of its committed listing (profiles/cosmul_digests.txt, taken at the parent commit, and the older
listings)."""
import os
import re
import shutil
import sys

import pytest

from conftest import REPO
from test_analogies_isa import QUERY_BAGS_LISTING
from test_cosmul_isa import ANALOGIES_LISTING
from test_query_bags_isa import QUERY_TOPK_LISTING
from test_query_matrix_isa import QUERIES_LISTING, kept
from test_query_topk_isa import QUERY_MATRIX_LISTING

sys.path.insert(0, os.path.join(REPO, 'tools', 'perf'))

pytestmark = pytest.mark.skipif(
    not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')), reason='hipcc not available')

COSMUL_LISTING = os.path.join(REPO, 'profiles', 'cosmul_digests.txt')   # tools/perf/isa.py --digests <COSMUL_SOURCE> of the parent commit
# eight wavefronts per SIMD (at most 64 vector registers, .sgpr_count at most 80)
WAVES = 8
REGISTERS = {'rank_count': (20, 35, 16), 'rank_fold': (21, 34, 0)}   # (vector registers, .sgpr_count, bytes of LDS)


@pytest.fixture(scope='module')
def unit():
    import isa
    return {name.replace('(anonymous namespace)::', '').split('(')[0]: facts
            for name, facts in isa.kernel_table(source=isa.RANKS_SOURCE).items()}


def test_the_unit_holds_two_kernels(unit):
    import isa
    assert sorted(unit) == ['rank_count', 'rank_fold']
    # a unit of its own, beside the fourteen of WITH_COSMUL
    assert isa.RANKS_SOURCE not in isa.WITH_COSMUL and len(isa.WITH_COSMUL) == 14
    assert isa.WITH_RANKS == isa.WITH_COSMUL + (isa.RANKS_SOURCE,)
    import build_native
    assert 'memb_hip_ranks.hip' in open(build_native.__file__).read()


def test_no_scratch_and_no_atomics(unit):
    for name, facts in unit.items():
        assert facts['private_segment'] == 0 and facts['scratch_ops'] == 0, name
        assert not re.search(r'^\s*(?:global|flat|buffer)_atomic', facts['code'], flags=re.M), name


def test_rank_count_loads_back_to_back_and_stores_once(unit):
    # COLUMNS_PER_THREAD loads with no wait and no branch between them, then the counting waits for them one by one
    header = open(os.path.join(REPO, 'memb_amd', 'csrc', 'hip_ranks.h')).read()
    per_thread = int(re.search(r'COLUMNS_PER_THREAD = (\d+);', header).group(1))
    code = unit['rank_count']['code']
    loads = [match.start() for match in re.finditer(r'^\s*global_load_dword\s', code, flags=re.M)]
    assert len(loads) == per_thread == 8
    between = code[loads[0]:loads[-1]]
    assert not re.search(r'vmcnt|^\s*s_cbranch|^\.LBB', between, flags=re.M)
    waits = re.findall(r'^\s*s_waitcnt vmcnt\((\d+)\)', code[loads[-1]:], flags=re.M)
    assert waits[:per_thread] == [str(count) for count in range(per_thread - 1, -1, -1)]
    # it ends in the one store of the block's partial count
    assert re.findall(r'^\s*global_store_(\w+)\s', code, flags=re.M) == ['dword']
    assert re.search(r'^\s*global_store_dword\s[^\n]*\n(?:\.LBB\w+:\s*\n)?\s*s_endpgm', code, flags=re.M)


def test_registers_are_what_the_design_states(unit):
    import isa
    design = open(os.path.join(REPO, 'DESIGN.md')).read()
    section = design[design.index('### 5.16'):]
    for name, (vgpr, sgpr_count, lds) in REGISTERS.items():
        facts = unit[name]
        assert (facts['vgpr'], facts['sgpr_count'], facts['lds']) == (vgpr, sgpr_count, lds), (name, facts['vgpr'], facts['sgpr_count'], facts['lds'])
        assert isa.waves_per_simd(facts['vgpr'], facts['sgpr_count']) == WAVES, name
        assert '| `{}` | {} | {} | {} | {} |'.format(name, vgpr, sgpr_count, WAVES, lds) in section, name   # the table's register columns


def test_the_cosmul_unit_keeps_its_digest():
    import isa
    kept(COSMUL_LISTING, (isa.COSMUL_SOURCE,), kernels=1)


def test_the_older_units_keep_their_digests():
    import isa
    kept(ANALOGIES_LISTING, (isa.ANALOGIES_SOURCE,), kernels=2)
    kept(QUERY_BAGS_LISTING, (isa.QUERY_BAGS_SOURCE,), kernels=3)
    kept(QUERY_TOPK_LISTING, (isa.QUERY_TOPK_SOURCE,), kernels=2)
    kept(QUERY_MATRIX_LISTING, (isa.QUERY_MATRIX_SOURCE,), kernels=3)
    kept(QUERIES_LISTING, (isa.QUERIES_SOURCE,), kernels=3)
    kept(os.path.join(REPO, 'profiles', 'norms_digests.txt'), isa.SOURCES)
    kept(os.path.join(REPO, 'profiles', 'pairs_digests.txt'), (isa.PAIRS_SOURCE,), kernels=4)
    kept(os.path.join(REPO, 'profiles', 'bag_pairs_digests.txt'), (isa.BAG_PAIRS_SOURCE,), kernels=3)
