"""What the compiler made of the kernels of memb_hip_pooled_chunked.hip (tools/perf/isa.py, source=POOLED_CHUNKED_SOURCE):
the checks tests/test_pooled_known_isa.py makes of its unit, and the registers DESIGN.md section 5.6 writes down."""
import os
import re
import shutil
import sys

import pytest

from conftest import REPO

sys.path.insert(0, os.path.join(REPO, 'tools', 'perf'))

needs_hipcc = pytest.mark.skipif(
    not (shutil.which('hipcc') or os.path.exists('/opt/rocm/bin/hipcc')), reason='hipcc not available')

# DESIGN.md section 5.6, "Registers", as written there: vector registers, .sgpr_count, LDS bytes
WRITTEN = {
    'chunk_block_sums': (28, 18, 2048),
    'chunk_scan_sums': (26, 30, 2048),
    'chunk_bag_starts': (42, 38, 2048),
    'chunk_offsets': (12, 22, 0),
    'pool_chunks<0>': (30, 76, 0),
    'pool_chunks<1>': (30, 76, 0),
    'pool_chunks<2>': (30, 76, 0),
}


@pytest.fixture(scope='module')
def kernels():
    import isa
    return {name.replace('(anonymous namespace)::', '').replace('void ', '').split('(')[0]: facts
            for name, facts in isa.kernel_table(source=isa.POOLED_CHUNKED_SOURCE).items()}


@pytest.fixture(scope='module')
def assembly():
    import isa
    return isa.device_assembly(source=isa.POOLED_CHUNKED_SOURCE)


@needs_hipcc
def test_the_chunked_kernels_exist(kernels):
    assert sorted(kernels) == sorted(WRITTEN), sorted(kernels)


@needs_hipcc
def test_chunked_kernels_spill_nothing_and_store_plainly(kernels, assembly):
    for name, facts in kernels.items():
        assert facts['private_segment'] == 0 and facts['scratch_ops'] == 0, (name, facts)
        assert facts['load_nt'] == 0 and facts['store_nt'] == 0, (name, facts)
    stores = re.findall(r'^\s*(?:global|flat|buffer)_store_\w+\s.*$', assembly, flags=re.M)
    assert stores and not [line for line in stores if re.search(r'\b(sc0|sc1|nt)\b', line)]
    # no atomics, and no block waits for another: the result is a function of the inputs alone
    assert not re.findall(r'^\s*(?:global|flat|buffer|ds)_atomic_\w+\s', assembly, flags=re.M)
    assert not re.findall(r'^\s*ds_\w+_rtn_\w+\s', assembly, flags=re.M)
    # the sums are single-lane v_add_f32: the packed forms flush subnormals on gfx950
    assert not re.findall(r'^\s*v_pk_\w+_f32\s', assembly, flags=re.M)
    assert len(re.findall(r'^\s*v_add_f32_e32\s', assembly, flags=re.M)) >= 3 * 16   # two unrolled batches per pool_chunks


@needs_hipcc
def test_chunked_kernels_keep_the_registers_written_down(kernels):
    import isa
    for name, (vgpr, sgpr, lds) in WRITTEN.items():
        facts = kernels[name]
        assert (facts['vgpr'], facts['sgpr_count'], facts['lds']) == (vgpr, sgpr, lds), (name, facts)
        assert isa.waves_per_simd(facts['vgpr'], facts['sgpr_count']) == 8, (name, facts)   # nothing here limits residency
