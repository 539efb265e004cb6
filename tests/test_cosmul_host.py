"""3CosMul without a GPU: the package's numpy scores against the scalar restatement of tests/cosmul_reference.py bit for
bit and against a float64 evaluation within the rounding bound, a device='cpu' reader's cosmul_topk, analogies_cosmul and
analogy_cosmul against their pieces and against an analogy worked out by hand, the argument errors, the C header and the
entry points' refusals, and hip_cosmul_launch.h's planning built into a program of its own under the host sanitizers."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from analogies_reference import topk_excluding_by_the_contract
from conftest import REPO
from cosmul_reference import (EPSILON, cosmul_score_of_one, cosmul_scores_by_the_contract, cosmul_scores_in_float64,
                              cosmul_topk_by_the_contract, questions_of)
from query_topk_reference import same_topk

HEADER = os.path.join(REPO, 'include', 'memb_hip_cosmul.h')
N_ROWS = 3000
PAIRS = ((0, 0), (1, 0), (0, 1), (2, 1), (1, 2), (3, 61), (64, 0), (0, 0))   # (positive, negative) terms of a question
FUSED = 'query_matrix_trained+cosmul_scores+topk_select_excluding+topk_merge'


def same_bits(got, want):
    return got.dtype == want.dtype == np.float32 and got.shape == want.shape and np.array_equal(got.view(np.uint32), want.view(np.uint32))


def test_the_restatement_by_hand():
    # 0.5, 0.0 and -0.5 positive, 1.0 negative: (0.75 * 0.5 * 0.25) / (1 + 1e-6f), every factor exact
    got = cosmul_score_of_one(np.array([0.5, 0.0, -0.5, 1.0], dtype=np.float32), 3)
    assert got == np.float32(np.float32(0.09375) / np.float32(np.float32(1) + EPSILON))
    assert EPSILON == np.float32(1e-6) and EPSILON.view(np.uint32) == 0x358637BD
    assert cosmul_score_of_one(np.zeros(0, dtype=np.float32), 0) == np.float32(1) / np.float32(np.float32(1) + EPSILON)
    assert cosmul_score_of_one(np.array([-1.0], dtype=np.float32), 1) == 0.0            # a positive term opposite: nothing
    with np.errstate(invalid='ignore'):
        assert np.isnan(cosmul_score_of_one(np.array([0.5, np.nan], dtype=np.float32), 1))
    # a negative term opposite: the epsilon alone divides
    assert cosmul_score_of_one(np.array([1.0, -1.0], dtype=np.float32), 1) == np.float32(np.float32(1) / EPSILON)


def test_the_packages_host_scores_are_the_restatement(native):
    from memb_amd.reader import cosmul_scores_host
    offsets, negatives_from, terms = questions_of(PAIRS)
    rng = np.random.default_rng(31)
    cosines = rng.uniform(-1, 1, size=(terms, 70)).astype(np.float32)
    cosines[:, :8] = np.array([-1.0, 1.0, np.float32(1) + np.float32(2.0 ** -23), np.nan, 0.0, -0.0, np.float32(-1) - np.float32(2.0 ** -23), 0.5],
                              dtype=np.float32)
    cosines[3::7, 9] = np.nan
    with np.errstate(invalid='ignore'):
        got, want = cosmul_scores_host(cosines, offsets, negatives_from), cosmul_scores_by_the_contract(cosines, offsets, negatives_from)
    assert same_bits(got, want)
    empty = np.float32(1) / np.float32(np.float32(1) + EPSILON)
    assert (got[[0, len(PAIRS) - 1]] == empty).all()                   # a question without terms, wherever it stands
    assert np.isnan(got[1:-1, 3]).all() and not np.isnan(got[:, 4]).any()
    assert cosmul_scores_host(cosines, [0], []).shape == (0, 70)
    assert cosmul_scores_host(cosines[:, :0], offsets, negatives_from).shape == (len(PAIRS), 0)
    for bad_offsets, bad_negatives in (([0, 2, 1], [0, 1]), ([0, terms + 1], [0]), ([-1, 2], [0]), ([0, 2], [3]), ([1, 2], [0]),
                                       ([0, 65], [0]), ([0, 2], [0, 1])):
        with pytest.raises(ValueError):
            cosmul_scores_host(cosines, bad_offsets, bad_negatives)


def test_the_host_scores_stay_within_the_rounding_bound(native):
    """Each of the at most 2T + 2 operations (T adds and T halvings -- exact, but counted --, T multiplies into num or den,
    the add of the epsilon and the divide) contributes a relative error of at most 2^-24; the bound is twice the
    first-order sum, (2T + 2) * 2^-23. Cosines in [-0.9, 1]: no factor below 0.05, so 64 of them stay above 1e-84 in
    float64 and above 2^-126 in float32 only where the product of 64 factors does -- the draw below is checked for it."""
    from memb_amd.reader import cosmul_scores_host
    offsets, negatives_from, terms = questions_of(PAIRS)
    cosines = np.random.default_rng(32).uniform(-0.9, 1, size=(terms, 500)).astype(np.float32)
    exact = cosmul_scores_in_float64(cosines, offsets, negatives_from)
    for scores in (cosmul_scores_host(cosines, offsets, negatives_from), cosmul_scores_by_the_contract(cosines, offsets, negatives_from)):
        assert np.isfinite(scores).all() and (scores >= np.float32(2.0 ** -126)).all()   # no intermediate underflowed
        for q, (positives, negatives) in enumerate(PAIRS):
            worst = float((np.abs(scores[q].astype(np.float64) - exact[q]) / exact[q]).max())
            bound = (2 * (positives + negatives) + 2) * 2.0 ** -23
            print('P {} N {}: worst relative error {:.3e}, bound {:.3e}'.format(positives, negatives, worst, bound))
            assert worst <= bound, (positives, negatives, worst, bound)


@pytest.fixture(scope='module')
def host_reader(native, make_model):
    path, words = make_model(N_ROWS, 300, 'trained', 4)
    return native.Reader(path, device='cpu'), words


def test_host_reader_selects_by_the_score(host_reader, monkeypatch):
    import memb_amd.reader
    reader, _ = host_reader
    monkeypatch.setattr(memb_amd.reader, 'NORMS_HOST_CHUNK', 16)   # bounded chunks: 53 candidates are four of them
    rows = np.random.default_rng(33).integers(0, N_ROWS, size=53).astype(np.uint32)
    rows[10:14] = rows[3] = 17                                       # repeated ids: ties across chunks
    rows[20] = 0xFFFFFFFF                                            # not in the model: cosine 0 against every term
    pairs = ((2, 1), (0, 0), (1, 0), (0, 2), (3, 3))
    offsets, negatives_from, count = questions_of(pairs)
    terms = reader.unit_rows_embedding(np.random.default_rng(34).integers(0, N_ROWS, size=count).astype(np.uint32))
    terms[offsets[2]] = reader.unit_rows_embedding(rows[3:4])[0]     # question 2's one term is candidate 3 itself
    matrix = reader.similarity_matrix(terms, rows)
    lists = np.full((len(pairs), 3), -1, dtype=np.int64)
    lists[2] = (11, 3, 40)                                           # among the tied best of question 2, in different chunks
    for k in (1, 10, 53, 64):
        for exclude in (None, lists):
            got = reader.cosmul_topk(terms, offsets, negatives_from, rows, k, exclude=exclude)
            assert same_topk(got, cosmul_topk_by_the_contract(matrix, offsets, negatives_from, k, exclude)), (k, exclude is None)
    assert reader.cosmul_topk(terms, offsets, negatives_from, rows, 3, exclude=lists)[1][2].tolist() == [10, 12, 13]
    empty = np.float32(1) / np.float32(np.float32(1) + EPSILON)
    values, positions = reader.cosmul_topk(terms, offsets, negatives_from, rows, 4)
    assert (values[1] == empty).all() and positions[1].tolist() == [0, 1, 2, 3]   # no term: every score equal, lower position first
    assert reader.cosmul_topk(terms, [0], [], rows, 4)[0].shape == (0, 4)
    none = reader.cosmul_topk(terms, offsets, negatives_from, rows[:0], 4)
    assert (none[1] == -1).all() and np.isneginf(none[0]).all()
    with pytest.raises(TypeError, match='float32'):
        reader.cosmul_topk(terms.astype(np.float64), offsets, negatives_from, rows, 3)
    with pytest.raises(ValueError, match='shape'):
        reader.cosmul_topk(terms[:, :299], offsets, negatives_from, rows, 3)
    with pytest.raises(ValueError, match='ascend'):
        reader.cosmul_topk(terms, offsets[::-1], negatives_from, rows, 3)
    with pytest.raises(ValueError, match='ascend'):
        reader.cosmul_topk(terms[:5], offsets, negatives_from, rows, 3)          # offsets beyond the terms
    with pytest.raises(ValueError, match='negatives_from'):
        reader.cosmul_topk(terms, offsets, negatives_from + 4, rows, 3)
    with pytest.raises(ValueError, match='64'):
        reader.cosmul_topk(np.zeros((65, 300), dtype=np.float32), [0, 65], [65], rows, 3)
    with pytest.raises(ValueError, match='64'):
        reader.cosmul_topk(terms, offsets, negatives_from, rows, 65)
    with pytest.raises(ValueError, match='shape'):
        reader.cosmul_topk(terms, offsets, negatives_from, rows, 3, exclude=lists[:2])
    with pytest.raises(RuntimeError, match="device 'cpu'"):
        reader.cosmul_topk_device(None, offsets, negatives_from, None, 3)
    assert reader.last_cosmul_kernel == ''


def test_host_reader_answers_cosmul_analogies(host_reader):
    reader, words = host_reader
    vocabulary = reader.keys()
    a, b, c, d = words[5], words[17], words[40], words[99]
    positive = [[b, c], [b, c, d], [a], [b, 'no such word é'], [], [c, c], []]
    negative = [[a], [a, d], [], [a], [], [], [a]]
    got = reader.analogies_cosmul(positive, negative, k=7)
    flat = [([b, c], [a]), ([b, c, d], [a, d]), ([a], []), None, None, ([c, c], []), ([], [a])]
    everything = np.arange(N_ROWS, dtype=np.uint32)
    for q, entries in enumerate(flat):
        if entries is None:
            assert got[q] == []
            continue
        own = reader.resolve_rows(entries[0] + entries[1])
        matrix = reader.similarity_matrix(reader.unit_rows_embedding(own), everything)
        scores = cosmul_scores_by_the_contract(matrix, [0, len(own)], [len(entries[0])])
        values, positions = topk_excluding_by_the_contract(scores, 7, [own.astype(np.int64)])
        assert got[q] == [(vocabulary[row], float(value)) for value, row in zip(values[0], positions[0])], q
        assert len(got[q]) == 7 and not {word for word, _ in got[q]} & set(entries[0] + entries[1])
    assert reader.analogy_cosmul(a, b, c, k=7) == got[0] and reader.analogy_cosmul(a, b, c) == got[0][:1]
    assert reader.analogies_cosmul([[b, c]], k=3) == reader.analogies_cosmul([[b, c]], None, 3) == reader.analogies_cosmul([[b, c]], [[]], 3)
    assert reader.analogies_cosmul([], [], 3) == []
    assert len(reader.analogies_cosmul([[b, c]], [[a]], k=64)[0]) == 64   # nothing reserved for the three dropped words
    # one positive word: the score rises with the cosine, so the words are most_similar's (the word itself left out there too)
    assert [word for word, _ in reader.analogies_cosmul([[a]], k=5)[0]] == [word for word, _ in reader.most_similar([a], k=5)[0]]
    with pytest.raises(TypeError, match='no weights'):
        reader.analogies_cosmul([[(b, 0.5), c]], [[a]])
    with pytest.raises(TypeError, match='no weights'):
        reader.analogies_cosmul([[b, c]], [[(a, -1.0)]])
    with pytest.raises(ValueError, match='64'):
        reader.analogies_cosmul([[a] * 40], [[b] * 25], 3)
    assert len(reader.analogies_cosmul([[a] * 40], [[b] * 24], 3)[0]) == 3
    with pytest.raises(ValueError, match='64'):
        reader.analogies_cosmul([[a]], k=65)
    with pytest.raises(ValueError, match='one list per query'):
        reader.analogies_cosmul([[a], [b]], [[c]])
    with pytest.raises(RuntimeError, match="device 'cpu'"):
        reader.analogies_cosmul_device([[a]])
    # the additive calls are what they were
    assert reader.analogy(a, b, c, k=3) == reader.analogies([[b, c]], [[a]], 3)[0]


def test_an_analogy_worked_out_by_hand(native, tmp_path):
    # axes: royal, male, female, other. king - man + woman; the scores below are (1 + cos) / 2 multiplied out by hand:
    #   queen   0.75    * 0.85355 / 0.5     = 1.28033      girl    0.53371 * 0.97673 / 0.54767 = 0.95183
    #   prince  0.97140 * 0.5     / 0.83333 = 0.58284      apple   0.5     * 0.5     / 0.5     = 0.5
    vectors = {'king': (1, 1, 0, 0), 'queen': (1, 0, 1, 0), 'man': (0, 1, 0, 0), 'woman': (0, 0, 1, 0), 'prince': (1, 1, 0, 0.5),
               'apple': (0, 0, 0, 1), 'girl': (0, 0.1, 1, 0.3)}
    builder = native.Builder(4, 'full', 32)
    builder.add_words(list(vectors), np.array(list(vectors.values()), dtype=np.float32))
    path = str(tmp_path / 'royal.bin')
    builder.save(path)
    reader = native.Reader(path, device='cpu')
    answer = reader.analogy_cosmul('man', 'king', 'woman', k=7)
    assert [word for word, _ in answer] == ['queen', 'girl', 'prince', 'apple']          # the three own words are no answers
    assert np.allclose([score for _, score in answer], [1.28033, 0.95183, 0.58284, 0.5], rtol=2e-5, atol=0)
    assert reader.analogies_cosmul([['king', 'woman'], ['king', 'nobody']], [['man'], []], k=2) == [answer[:2], []]


# ---- the C side ----

def test_header_is_plain_c_and_cxx():
    for compiler, flags in (('gcc', ['-std=c99', '-pedantic', '-Wall', '-Werror', '-x', 'c']),
                            ('g++', ['-std=c++14', '-Wall', '-Werror', '-x', 'c++'])):
        result = subprocess.run([compiler, *flags, '-fsyntax-only', HEADER], stdout=subprocess.PIPE,
                                stderr=subprocess.STDOUT, text=True)
        assert result.returncode == 0, result.stdout
    text = open(HEADER).read()
    assert '#include "memb_hip_query_matrix.h"' in text and '#define MEMB_HIP_COSMUL_MAX_TERMS 64' in text
    assert 'num / (den + 1e-6f)' in text and 'never a fused multiply-add' in text
    for word in ('ReadersUnion', 'ShardedReader', 'bf16 / fp16', 'k > 64', 'more than 64\n * terms', 'weights',
                 'fused into the selection kernel', 'pooled-bag'):
        assert word in text, word
    # the names the older headers' tests keep to their own header
    for word in ('query_topk', 'dense_topk', 'TOPK', 'query_bags', 'excluding', 'weighted_rows_sum', 'analogies'):
        assert word not in text, word
    # no older header knows the new names, and the analogies header still says what it left out
    for name in sorted(os.listdir(os.path.join(REPO, 'include'))):
        if name != 'memb_hip_cosmul.h':
            older = open(os.path.join(REPO, 'include', name)).read()
            assert 'memb_hip_cosmul' not in older and 'cosmul_scores' not in older and 'COSMUL' not in older, name
    assert 'Not built: 3CosMul scoring' in open(os.path.join(REPO, 'include', 'memb_hip_analogies.h')).read()


def test_entry_points_are_exported_and_refuse_bad_arguments(native):
    library = ctypes.CDLL(native.HIP_LIBRARY_PATH)
    library.memb_hip_last_error.restype = ctypes.c_char_p
    pointer, size = ctypes.c_void_p, ctypes.c_size_t
    invalid = 1   # MEMB_HIP_ERR_INVALID

    def refused(code, word):
        message = library.memb_hip_last_error()
        return code == invalid and message and word in message

    scores = library.memb_hip_cosmul_scores_device
    scores.argtypes = [ctypes.c_int, pointer, size, pointer, pointer, size, size, pointer, size, pointer]
    # (every one of these is refused before a pointer is read or the device is touched)
    assert refused(scores(-1, 64, 8, 128, 256, 2, 7, 512, 8, None), b'device')
    assert refused(scores(0, 64, 8, None, 256, 2, 7, 512, 8, None), b'null')
    assert refused(scores(0, 64, 8, 128, None, 2, 7, 512, 8, None), b'null')
    assert refused(scores(0, 64, 8, 128, 256, 2, 7, None, 8, None), b'null')
    assert refused(scores(0, None, 8, 128, 256, 2, 7, 512, 8, None), b'cosines')
    assert refused(scores(0, 64, 6, 128, 256, 2, 7, 512, 8, None), b'at least n')
    assert refused(scores(0, 64, 8, 128, 256, 2, 7, 512, 6, None), b'at least n')
    for shifted in ((66, 128, 256, 512), (64, 130, 256, 512), (64, 128, 257, 512), (64, 128, 256, 515)):
        assert refused(scores(0, shifted[0], 8, shifted[1], shifted[2], 2, 7, shifted[3], 8, None), b'aligned'), shifted
    assert refused(scores(0, 64, 8, 128, 256, 2 ** 16 + 1, 7, 512, 8, None), b'too large')
    assert refused(scores(0, 64, 2 ** 32, 128, 256, 2, 2 ** 31 + 1, 512, 2 ** 32, None), b'too large')
    assert scores(0, 64, 8, 128, 256, 0, 7, 512, 8, None) == 0      # no question: a no-op, nothing touched
    assert scores(0, None, 0, 128, 256, 2, 0, 512, 0, None) == 0    # no column likewise
    nearest = library.memb_hip_query_cosmul_nearest_device
    nearest.argtypes = [pointer, pointer, size, size, pointer, pointer, size, pointer, size, ctypes.c_uint32, pointer, size, size,
                        pointer, pointer, size, pointer, size, pointer]
    assert refused(nearest(None, 64, 3, 300, 128, 256, 1, 512, 5, 3, None, 0, 0, 1024, 2048, 3, 4096, 1 << 20, None), b'ctx')
    size_of = library.memb_hip_query_cosmul_workspace_bytes
    size_of.restype = size
    size_of.argtypes = [pointer, size, size, size, ctypes.c_uint32, ctypes.c_int]
    assert size_of(None, 3, 1, 1000, 10, 0) == 0
    name = library.memb_hip_query_cosmul_kernel_name
    name.restype = ctypes.c_char_p
    name.argtypes = [pointer]
    assert name(None) == b'cosmul_scores'

    import memb_amd
    from memb_amd import _memb, _memb_cosmul
    # the bindings: a module of its own, by context handle; a reader on the host has no context
    for name in ('cosmul_scores_to_device', 'query_cosmul_nearest_to_device', 'query_cosmul_workspace_bytes', 'query_cosmul_kernel_name'):
        assert callable(getattr(_memb_cosmul, name)), name
    assert _memb_cosmul.cosmul_scores_kernel_name() == 'cosmul_scores'
    assert _memb_cosmul.query_cosmul_kernel_name(0) == '' and _memb_cosmul.query_cosmul_workspace_bytes(0, 3, 1, 1000, 10) == 0
    with pytest.raises(RuntimeError, match='memb_hip_query_cosmul_nearest_device.*ctx'):
        _memb_cosmul.query_cosmul_nearest_to_device(0, 64, 3, 300, 128, 256, 1, 512, 5, 3, 0, 0, 0, 1024, 2048, 3, 4096, 1 << 20)
    with pytest.raises(RuntimeError, match='memb_hip_cosmul_scores_device.*device'):
        _memb_cosmul.cosmul_scores_to_device(-1, 64, 8, 128, 256, 2, 7, 512, 8)
    assert memb_amd.COSMUL_MAX_TERMS == _memb_cosmul.COSMUL_MAX_TERMS == 64 == _memb.QUERY_TOPK_MAX_EXCLUDED
    assert not [name for name in dir(_memb) + dir(_memb.Reader) if 'cosmul' in name.lower()]   # (the surface of _memb is pinned)
    for method in ('cosmul_topk_device', 'cosmul_topk', 'analogies_cosmul_device', 'analogies_cosmul', 'analogy_cosmul', 'last_cosmul_kernel'):
        assert hasattr(native.Reader, method)
    assert callable(memb_amd.reader.cosmul_scores_host)


def _hipcc():
    for candidate in (shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if candidate and os.path.exists(candidate):
            return candidate
    return None


@pytest.mark.skipif(not _hipcc(), reason='hipcc not available')
def test_planning_under_the_host_sanitizers(tmp_path):
    # hip_cosmul_launch.h's first part as a program of its own with AddressSanitizer and UndefinedBehaviorSanitizer on the
    # HOST code: no GPU, no Python inside
    source = os.path.join(REPO, 'tests', 'cpp', 'cosmul_planning_main.cpp')
    program = str(tmp_path / 'cosmul_planning')
    build = subprocess.run(
        [_hipcc(), '-x', 'c++', '-std=c++17', '-O1', '-g', '-Xarch_host', '-fsanitize=address,undefined',
         '-fno-sanitize-recover=all', '-o', program, source],
        stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert build.returncode == 0, build.stdout
    run = subprocess.run([program], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert run.returncode == 0 and 'cosmul planning: ok' in run.stdout, run.stdout
