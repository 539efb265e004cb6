"""What the compiler made of the kernels: per kernel the loads / stores by cache policy, LDS-DMA loads,
registers, scratch and LDS, read from the device assembly (no GPU needed).

    python tools/perf/isa.py [substring of the demangled kernel name] [-- extra hipcc flags]
    python tools/perf/isa.py --digests     one line per kernel of every translation unit of libmemb_hip.so (WITH_WITHIN),
                                           instruction digest and resources: run it on two commits and diff the listings
                                           to see which kernels a change touched

tests/test_isa.py uses kernel_table() to pin facts a source-level reading can get wrong: round 2 shipped
`flag ? *p : __builtin_nontemporal_load(p)`, which LLVM folds into ONE plain load, and reported the
`nt` loads as adopted.
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
SOURCE = os.path.join(REPO, 'memb_amd', 'csrc', 'memb_hip.hip')
NARROW_SOURCE = os.path.join(REPO, 'memb_amd', 'csrc', 'memb_hip_narrow.hip')
POOLED_SOURCE = os.path.join(REPO, 'memb_amd', 'csrc', 'memb_hip_pooled.hip')
POOLED_CHUNKED_SOURCE = os.path.join(REPO, 'memb_amd', 'csrc', 'memb_hip_pooled_chunked.hip')
POOLED_UNION_SOURCE = os.path.join(REPO, 'memb_amd', 'csrc', 'memb_hip_pooled_union.hip')
NORMS_SOURCE = os.path.join(REPO, 'memb_amd', 'csrc', 'memb_hip_norms.hip')
SOURCES = (SOURCE, NARROW_SOURCE, POOLED_SOURCE, POOLED_CHUNKED_SOURCE, POOLED_UNION_SOURCE, NORMS_SOURCE)   # every translation unit of build_native.build_hip_library
# the pair kernels' unit, kept out of SOURCES (tests/test_norms_isa.py counts the units that existed before it there);
# ALL_SOURCES is what --digests listed before the bag-pair unit
PAIRS_SOURCE = os.path.join(REPO, 'memb_amd', 'csrc', 'memb_hip_pairs.hip')
ALL_SOURCES = SOURCES + (PAIRS_SOURCE,)
# the bag-pair kernels' unit, kept out of ALL_SOURCES likewise (tests/test_pairs_isa.py pins it); LIBRARY_SOURCES is every
# translation unit of the library before the query unit, and what --digests listed then
BAG_PAIRS_SOURCE = os.path.join(REPO, 'memb_amd', 'csrc', 'memb_hip_bag_pairs.hip')
LIBRARY_SOURCES = ALL_SOURCES + (BAG_PAIRS_SOURCE,)
# the query kernel's unit, kept out of LIBRARY_SOURCES likewise (tests/test_bag_pairs_isa.py pins it); EVERY_SOURCE is every
# translation unit of the library before the query-matrix unit, and what --digests listed then
QUERIES_SOURCE = os.path.join(REPO, 'memb_amd', 'csrc', 'memb_hip_queries.hip')
EVERY_SOURCE = LIBRARY_SOURCES + (QUERIES_SOURCE,)
# the query-matrix kernel's unit, kept out of EVERY_SOURCE likewise (tests/test_queries_isa.py pins it); WHOLE_LIBRARY is
# every translation unit of the library, and what --digests lists
QUERY_MATRIX_SOURCE = os.path.join(REPO, 'memb_amd', 'csrc', 'memb_hip_query_matrix.hip')
WHOLE_LIBRARY = EVERY_SOURCE + (QUERY_MATRIX_SOURCE,)
# the selection kernels' unit, kept out of WHOLE_LIBRARY likewise (tests/test_query_matrix_isa.py pins it); WITH_QUERY_TOPK
# is every translation unit of the library before the query-bags unit
QUERY_TOPK_SOURCE = os.path.join(REPO, 'memb_amd', 'csrc', 'memb_hip_query_topk.hip')
WITH_QUERY_TOPK = WHOLE_LIBRARY + (QUERY_TOPK_SOURCE,)
# the query-bags kernel's unit, kept out of WITH_QUERY_TOPK likewise (tests/test_query_topk_isa.py pins it); WITH_QUERY_BAGS
# is every translation unit of the library before the analogies unit
QUERY_BAGS_SOURCE = os.path.join(REPO, 'memb_amd', 'csrc', 'memb_hip_query_bags.hip')
WITH_QUERY_BAGS = WITH_QUERY_TOPK + (QUERY_BAGS_SOURCE,)
# the unit of the selection with exclusion lists and of the weighted sums, kept out of WITH_QUERY_BAGS likewise
# (tests/test_query_bags_isa.py pins it); WITH_ANALOGIES is every translation unit of the library before the 3CosMul unit
ANALOGIES_SOURCE = os.path.join(REPO, 'memb_amd', 'csrc', 'memb_hip_analogies.hip')
WITH_ANALOGIES = WITH_QUERY_BAGS + (ANALOGIES_SOURCE,)
# the unit of the 3CosMul scores, kept out of WITH_ANALOGIES likewise (tests/test_analogies_isa.py pins it); WITH_COSMUL is
# every translation unit of the library before the rank-count unit
COSMUL_SOURCE = os.path.join(REPO, 'memb_amd', 'csrc', 'memb_hip_cosmul.hip')
WITH_COSMUL = WITH_ANALOGIES + (COSMUL_SOURCE,)
# the unit of the rank counts, kept out of WITH_COSMUL likewise (tests/test_cosmul_isa.py pins it); WITH_RANKS is every
# translation unit of the library before the unit of the lists
RANKS_SOURCE = os.path.join(REPO, 'memb_amd', 'csrc', 'memb_hip_ranks.hip')
WITH_RANKS = WITH_COSMUL + (RANKS_SOURCE,)
# the unit of the lists of the candidates before a mark, kept out of WITH_RANKS likewise (tests/test_ranks_isa.py pins it);
# WITH_WITHIN is every translation unit of the library today, and what --digests lists
WITHIN_SOURCE = os.path.join(REPO, 'memb_amd', 'csrc', 'memb_hip_within.hip')
WITH_WITHIN = WITH_RANKS + (WITHIN_SOURCE,)
# the flags of build_native.build_hip_library
FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-ffp-contract=off', '-fhip-fp32-correctly-rounded-divide-sqrt',
         '-Wno-unused-value', '-Wno-align-mismatch', '-Wno-pass-failed', '-Wno-unused-command-line-argument']


def _tool(name):
    for candidate in (shutil.which(name), '/opt/rocm/bin/' + name, '/opt/rocm/lib/llvm/bin/' + name, '/usr/bin/' + name):
        if candidate and os.path.exists(candidate):
            return candidate
    raise RuntimeError(name + ' not found')


def device_assembly(extra_flags=(), source=SOURCE):
    with tempfile.TemporaryDirectory() as scratch:
        target = os.path.join(scratch, 'memb_hip.s')
        subprocess.run([_tool('hipcc'), *FLAGS, *extra_flags, '--cuda-device-only', '-S', '-o', target, source],
                       check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        with open(target) as f:
            return f.read()


def _instructions(code, symbol):
    """A kernel's instructions and labels as text that does not depend on the translation unit the kernel lives in or on
    its place there: without the kernel's own symbol, the function number of its labels (.LBB<n>_<m>, .Lfunc_end<n>) and
    the compiler's comments, which repeat that number (`; in Loop: Header=BB<n>_<m>`) behind padding as wide as the label"""
    code = re.sub(r'\.(LBB|Lfunc_begin|Lfunc_end)\d+', r'.\1', code.replace(symbol, 'KERNEL'))
    lines = (re.sub(r'\s*;.*$', '', line) for line in code.split('\n'))
    return '\n'.join(line for line in lines if line.strip())


def kernel_table(extra_flags=(), source=SOURCE):
    """{demangled kernel name: facts} for every kernel of one translation unit of libmemb_hip.so (default memb_hip.hip;
    NARROW_SOURCE: the bf16 / fp16 decode kernels; POOLED_SOURCE: every sequential pooled kernel; POOLED_CHUNKED_SOURCE: the
    chunked order's; POOLED_UNION_SOURCE: the pooled kernels of averaged unions and of dense rows; NORMS_SOURCE: row norms and unit rows; PAIRS_SOURCE: the cosine of row pairs; BAG_PAIRS_SOURCE: the cosine of pairs of pooled bags; QUERIES_SOURCE: the cosine of query vectors against groups of rows; QUERY_MATRIX_SOURCE: the cosine of every query against one shared list of rows; QUERY_TOPK_SOURCE: the k best columns of every row of a matrix; QUERY_BAGS_SOURCE: the cosine of every query against every pooled bag of rows; ANALOGIES_SOURCE: the selection with exclusion lists and sums of weighted rows; COSMUL_SOURCE: the 3CosMul scores; RANKS_SOURCE: the number of candidates that precede a mark; WITHIN_SOURCE: the list of those candidates; or any other path, such as a unit of another checkout)"""
    text = device_assembly(extra_flags, source)
    names = re.findall(r'^\s*\.amdhsa_kernel (\S+)$', text, flags=re.M)
    demangled = subprocess.run([_tool('c++filt')], input='\n'.join(names), stdout=subprocess.PIPE, text=True,
                               check=True).stdout.split('\n')
    table = {}
    for name, pretty in zip(names, demangled):
        start = text.index('\n' + name + ':')
        body = text[start:text.index('.amdhsa_kernel ' + name, start)]
        code = body.split('.section')[0]
        descriptor = text[text.index('.amdhsa_kernel ' + name):]
        descriptor = descriptor[:descriptor.index('.end_amdhsa_kernel')]

        def field(key, where=descriptor):
            match = re.search(r'\.' + key + r'\s+(\d+)', where)
            return int(match.group(1)) if match else None

        metadata = re.search(r'\.name:\s+' + re.escape(name) + r'\n(.*?)\n  - ', text + '\n  - ', flags=re.S)
        meta = metadata.group(1) if metadata else ''
        loads = re.findall(r'^\s*global_load_dwordx4\s.*$', code, flags=re.M)
        stores = re.findall(r'^\s*global_store_dwordx4\s.*$', code, flags=re.M)
        any_loads = re.findall(r'^\s*(?:global|flat|buffer)_load_\w+\s.*$', code, flags=re.M)
        any_stores = re.findall(r'^\s*(?:global|flat|buffer)_store_\w+\s.*$', code, flags=re.M)
        table[pretty] = {
            'symbol': name,
            'load_x4': len(loads),
            'load_x4_nt': sum(1 for line in loads if re.search(r'\bnt\b', line)),
            'store_x4': len(stores),
            'store_x4_nt': sum(1 for line in stores if re.search(r'\bnt\b', line)),
            # of EVERY width (round 4's test counted x4 loads only and missed a non-temporal dword load)
            'load_nt': sum(1 for line in any_loads if re.search(r'\bnt\b', line)),
            'store_nt': sum(1 for line in any_stores if re.search(r'\bnt\b', line)),
            'lds_dma': len(re.findall(r'^\s*(global|buffer)_load_lds_\w+', code, flags=re.M)) +
                       len(re.findall(r'^\s*buffer_load_\w+ .*\blds\b', code, flags=re.M)),
            'scratch_ops': len(re.findall(r'^\s*scratch_(load|store)_', code, flags=re.M)),
            'vgpr': field('amdhsa_next_free_vgpr'),
            'sgpr': field('amdhsa_next_free_sgpr'),
            'accum_offset': field('amdhsa_accum_offset'),
            'private_segment': field('amdhsa_private_segment_fixed_size'),
            'lds': field('amdhsa_group_segment_fixed_size'),
            'code': code,
            'digest': hashlib.sha256(_instructions(code, name).encode()).hexdigest()[:16],
            'vgpr_count': field('vgpr_count:', meta) if meta else None,
            # (.sgpr_count of the metadata = next_free_sgpr + VCC / flat scratch / XNACK: what the hardware allocates by)
            'sgpr_count': field('sgpr_count:', meta) if meta else None,
        }
    return table


def kernel_digests(sources=SOURCES):
    """{demangled kernel name: (digest of its instructions, vgpr, sgpr_count, LDS bytes, scratch bytes)} over every
    translation unit of the library (or the units given): equal before and after a change that is meant to leave the device
    code alone, wherever it moves a kernel"""
    return {pretty: (facts['digest'], facts['vgpr'], facts['sgpr_count'], facts['lds'], facts['private_segment'])
            for source in sources for pretty, facts in kernel_table(source=source).items()}


def waves_per_simd(vgpr, sgpr_count=None):
    """MI355X_MICROARCH.md: vector registers -- allocation granule 8, 512 per lane per SIMD; scalar registers
    ('Residency and cooperative launch') -- 800 per SIMD, granule 16 plus 16: .sgpr_count <= 80 -> 8 wavefronts, 81-96 -> 7,
    97-112 -> 6 (the compiler's own `; Occupancy:` line does not know the second rule)."""
    allocated = (vgpr + 7) // 8 * 8
    waves = min(8, 512 // max(allocated, 8))
    if sgpr_count:
        waves = min(waves, 800 // ((sgpr_count + 15) // 16 * 16 + 16))
    return waves


if __name__ == '__main__':
    arguments = sys.argv[1:]
    extra = []
    if '--' in arguments:
        extra = arguments[arguments.index('--') + 1:]
        arguments = arguments[:arguments.index('--')]
    if arguments[:1] == ['--digests']:   # one line per kernel, to diff against another commit's; [units of that commit]
        for pretty, facts in sorted(kernel_digests(arguments[1:] or WITH_WITHIN).items()):
            print(pretty.replace('(anonymous namespace)::', '').split('(')[0], *facts)
        sys.exit(0)
    needle = arguments[0] if arguments else ''
    print('%-92s %5s %5s %4s %6s %6s %4s %4s %7s %8s' % (
        'kernel', 'ld.x4', 'nt', 'dma', 'st.x4', 'st.nt', 'vgpr', 'sgpr', 'scratch', 'waves/EU'))   # sgpr = .sgpr_count
    for pretty, facts in sorted(kernel_table(extra).items()):
        if needle in pretty:
            short = pretty.replace('(anonymous namespace)::', '').split('(')[0]
            print('%-92s %5d %5d %4d %6d %6d %4d %4d %7d %8d' % (
                short[:92], facts['load_x4'], facts['load_x4_nt'], facts['lds_dma'], facts['store_x4'], facts['store_x4_nt'],
                facts['vgpr'], facts['sgpr_count'] or facts['sgpr'], facts['private_segment'], waves_per_simd(facts['vgpr'], facts['sgpr_count'])))
