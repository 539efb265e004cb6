"""What the compiler made of memb_hip_cosmul.hip (tools/perf/isa.py, source=COSMUL_SOURCE), without a GPU: one kernel, no
scratch, no LDS, no atomics, the registers and wavefronts per SIMD DESIGN.md section 5.15 states, separately rounded
multiplies and adds with no fused multiply-add among the contract's operations, the term loads issued ahead of the
multiply chain -- and every kernel of the units that existed before keeps the digest of its committed listing
(profiles/analogies_digests.txt, taken at the parent commit, and the older listings)."""
import os
import re
import shutil
import sys

import pytest

from conftest import REPO
from test_analogies_isa import QUERY_BAGS_LISTING
from test_query_bags_isa import QUERY_TOPK_LISTING
from test_query_matrix_isa import QUERIES_LISTING, kept
from test_query_topk_isa import QUERY_MATRIX_LISTING

sys.path.insert(0, os.path.join(REPO, 'tools', 'perf'))

pytestmark = pytest.mark.skipif(
    not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')), reason='hipcc not available')

ANALOGIES_LISTING = os.path.join(REPO, 'profiles', 'analogies_digests.txt')   # tools/perf/isa.py --digests <ANALOGIES_SOURCE> of the parent commit
# eight wavefronts per SIMD (at most 64 vector registers, .sgpr_count at most 80)
WAVES = 8
REGISTERS = {'cosmul_scores': (12, 28)}   # (vector registers, .sgpr_count)
FUSED = r'^\s*v_(?:pk_)?(?:fma|fmac|mad|mac)_(?:legacy_)?f\d+'   # (v_mad_u64_u32 is an address)


@pytest.fixture(scope='module')
def unit():
    import isa
    return {name.replace('(anonymous namespace)::', '').split('(')[0]: facts
            for name, facts in isa.kernel_table(source=isa.COSMUL_SOURCE).items()}


def test_the_unit_holds_one_kernel(unit):
    import isa
    assert sorted(unit) == ['cosmul_scores']
    # a unit of its own, beside the thirteen of WITH_ANALOGIES
    assert isa.COSMUL_SOURCE not in isa.WITH_ANALOGIES and len(isa.WITH_ANALOGIES) == 13
    assert isa.WITH_COSMUL == isa.WITH_ANALOGIES + (isa.COSMUL_SOURCE,)
    import build_native
    assert 'memb_hip_cosmul.hip' in open(build_native.__file__).read()


def test_no_scratch_no_lds_no_atomics(unit):
    facts = unit['cosmul_scores']
    assert facts['private_segment'] == 0 and facts['scratch_ops'] == 0, facts['private_segment']
    assert facts['lds'] == 0 and not re.search(r'^\s*ds_(?:read|write)', facts['code'], flags=re.M)
    assert not re.search(r'^\s*(?:global|flat|buffer)_atomic', facts['code'], flags=re.M)
    assert re.findall(r'^\s*global_store_(\w+)\s', facts['code'], flags=re.M) == ['dword']   # one score


def test_rounded_multiplies_and_adds_and_no_fused_multiply_add(unit):
    """The contract's adds and multiplies are v_add_f32 and v_mul_f32. The one place a fused multiply-add may stand is the
    compiler's expansion of the correctly rounded divide (v_div_scale_f32 ... v_div_fixup_f32: a reciprocal refined by
    fused steps is how the hardware divides to the last bit; there is no division instruction to ask for instead), so the
    code is cut there: none before the first v_div_scale_f32, none behind the v_div_fixup_f32, and exactly one divide."""
    code = unit['cosmul_scores']['code']
    assert re.search(r'^\s*v_mul_f32', code, flags=re.M) and re.search(r'^\s*v_add_f32', code, flags=re.M)
    assert len(re.findall(r'^\s*v_div_fixup_f32', code, flags=re.M)) == 1 and len(re.findall(r'^\s*v_div_fmas_f32', code, flags=re.M)) == 1
    start = re.search(r'^\s*v_div_scale_f32', code, flags=re.M).start()
    end = re.search(r'^\s*v_div_fixup_f32.*$', code, flags=re.M).end()
    assert start < end
    assert not re.search(FUSED, code[:start], flags=re.M) and not re.search(FUSED, code[end:], flags=re.M)
    # (no approximate float divide; v_rcp_iflag_f32 is the integer division of the block index by blocksPerQuestion)
    assert not re.search(r'^\s*v_rcp_f32', code[:start] + code[end:], flags=re.M)
    # the epsilon is float32(0.000001), added to den by one v_add_f32 right before the divide
    assert re.search(r'^\s*v_add_f32_e32 v\d+, 0x358637bd, v\d+\s*\n\s*v_div_scale_f32', code, flags=re.M)


def test_the_term_loads_are_issued_ahead_of_the_multiplies(unit):
    # TERMS_IN_FLIGHT loads with no wait and no branch between them, then the chain waits for them one by one
    header = open(os.path.join(REPO, 'memb_amd', 'csrc', 'hip_cosmul.h')).read()
    in_flight = int(re.search(r'TERMS_IN_FLIGHT = (\d+);', header).group(1))
    code = unit['cosmul_scores']['code']
    loads = [match.start() for match in re.finditer(r'^\s*global_load_dword\s', code, flags=re.M)]
    assert len(loads) == in_flight == 4
    between = code[loads[0]:loads[-1]]
    assert not re.search(r'vmcnt|^\s*s_cbranch|^\.LBB', between, flags=re.M)
    waits = re.findall(r'^\s*s_waitcnt vmcnt\((\d+)\)', code[loads[-1]:], flags=re.M)
    assert waits[:in_flight] == [str(count) for count in range(in_flight - 1, -1, -1)]


def test_registers_are_what_the_design_states(unit):
    import isa
    design = open(os.path.join(REPO, 'DESIGN.md')).read()
    section = design[design.index('### 5.15'):]
    for name, (vgpr, sgpr_count) in REGISTERS.items():
        facts = unit[name]
        assert (facts['vgpr'], facts['sgpr_count']) == (vgpr, sgpr_count), (name, facts['vgpr'], facts['sgpr_count'])
        assert isa.waves_per_simd(facts['vgpr'], facts['sgpr_count']) == WAVES, name
        assert '| `{}` | {} | {} | {} | 0 |'.format(name, vgpr, sgpr_count, WAVES) in section, name   # the table's register columns


def test_the_analogies_unit_keeps_its_digests():
    import isa
    kept(ANALOGIES_LISTING, (isa.ANALOGIES_SOURCE,), kernels=2)


def test_the_older_units_keep_their_digests():
    import isa
    kept(QUERY_BAGS_LISTING, (isa.QUERY_BAGS_SOURCE,), kernels=3)
    kept(QUERY_TOPK_LISTING, (isa.QUERY_TOPK_SOURCE,), kernels=2)
    kept(QUERY_MATRIX_LISTING, (isa.QUERY_MATRIX_SOURCE,), kernels=3)
    kept(QUERIES_LISTING, (isa.QUERIES_SOURCE,), kernels=3)
    kept(os.path.join(REPO, 'profiles', 'norms_digests.txt'), isa.SOURCES)
    kept(os.path.join(REPO, 'profiles', 'pairs_digests.txt'), (isa.PAIRS_SOURCE,), kernels=4)
    kept(os.path.join(REPO, 'profiles', 'bag_pairs_digests.txt'), (isa.BAG_PAIRS_SOURCE,), kernels=3)
