"""The argument check every pooled entry point of libmemb_hip.so shares (hip_pooled_launch.h: PooledCall::check), through the C ABI
without compute, in test_cabi.py's style: one argument per call is made wrong, and every entry point must refuse it with
MEMB_HIP_ERR_INVALID and the same memb_hip_last_error() text; two mistakes at once show which check comes first. The texts
are those of the entry points as they were written one by one, before they shared the check. No context is dereferenced
before the null check has passed and none of these calls passes it, so a fake one serves; no device is needed."""
import ctypes

import pytest

OK, INVALID = 0, 1
F32, BF16 = 0, 1          # MEMB_HIP_OUT_*
SUM, MEAN = 0, 1          # MEMB_HIP_POOL_*
BAD_OUT_TYPE, BAD_MODE = 7, 5
UNKNOWN_OUT_TYPE = 'unknown out_type 7'
UNKNOWN_MODE = 'unknown pooling mode 5'
NULL_ARGUMENT = 'null argument'
LD_TOO_SMALL = 'ld must be at least col_off + dim'
DENSE_UNALIGNED = 'values and out must be aligned to their elements'
DENSE_DIM = 'dim must be 1 .. 2^32 - 1, ld_values at least dim and device a HIP device'

P, Z, I = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
FAKE = 64   # a pointer that is never followed: a context, rows, offsets or out that only has to be there


@pytest.fixture(scope='module')
def entry_points(native):
    """{name: call(out_type, mode, offsets) -> (code, text)} for the six entry points: one bag of four entries, every other
    argument well-formed"""
    library = ctypes.CDLL(native.HIP_LIBRARY_PATH)
    library.memb_hip_last_error.restype = ctypes.c_char_p
    for name in ('memb_hip_abi_version', 'memb_hip_pool_rows_device', 'memb_hip_pool_rows_device_typed',
                 'memb_hip_pool_known_rows_device_typed', 'memb_hip_pool_rows_union_device', 'memb_hip_pool_dense_rows_device',
                 'memb_hip_pool_rows_chunked_device_typed'):
        assert hasattr(library, name), name
    library.memb_hip_pool_rows_device.argtypes = [P, P, Z, P, Z, P, Z, Z, I, P]
    library.memb_hip_pool_rows_device_typed.argtypes = [P, P, Z, P, Z, P, I, Z, Z, I, P]
    library.memb_hip_pool_known_rows_device_typed.argtypes = [P, P, Z, P, Z, P, I, Z, Z, I, P, P]
    library.memb_hip_pool_rows_union_device.argtypes = [P, P, Z, Z, P, Z, P, I, Z, Z, I, P]
    library.memb_hip_pool_dense_rows_device.argtypes = [I, P, Z, Z, Z, P, Z, P, I, Z, Z, I, P]
    library.memb_hip_pool_rows_chunked_device_typed.argtypes = [P, P, Z, P, Z, P, I, Z, Z, I, I, P, P, Z, P]
    contexts = (P * 2)(FAKE, FAKE)     # host arrays of a union of two: the entries are never followed
    row_arrays = (P * 2)(FAKE, FAKE)

    def answer(code):
        return code, library.memb_hip_last_error().decode()

    calls = {
        'memb_hip_pool_rows_device_typed': lambda out_type, mode, offsets: answer(
            library.memb_hip_pool_rows_device_typed(FAKE, FAKE, 4, offsets, 1, FAKE, out_type, 8, 0, mode, None)),
        'memb_hip_pool_known_rows_device_typed': lambda out_type, mode, offsets: answer(
            library.memb_hip_pool_known_rows_device_typed(FAKE, FAKE, 4, offsets, 1, FAKE, out_type, 8, 0, mode, None, None)),
        'memb_hip_pool_rows_union_device': lambda out_type, mode, offsets: answer(
            library.memb_hip_pool_rows_union_device(contexts, row_arrays, 2, 4, offsets, 1, FAKE, out_type, 8, 0, mode, None)),
        'memb_hip_pool_dense_rows_device': lambda out_type, mode, offsets: answer(
            library.memb_hip_pool_dense_rows_device(0, FAKE, 4, 8, 8, offsets, 1, FAKE, out_type, 8, 0, mode, None)),
        'memb_hip_pool_rows_chunked_device_typed': lambda out_type, mode, offsets: answer(
            library.memb_hip_pool_rows_chunked_device_typed(
                FAKE, FAKE, 4, offsets, 1, FAKE, out_type, 8, 0, mode, 0, None, FAKE, 1 << 20, None)),
    }

    def untyped(out_type, mode, offsets):   # (float rows only: it has no out_type to get wrong)
        assert out_type == F32
        return answer(library.memb_hip_pool_rows_device(FAKE, FAKE, 4, offsets, 1, FAKE, 8, 0, mode, None))

    calls['memb_hip_pool_rows_device'] = untyped
    return library, calls


def test_every_pooled_entry_point_refuses_the_same_mistake_with_the_same_text(entry_points):
    _, calls = entry_points
    assert len(calls) == 6
    for name, call in calls.items():
        typed = name != 'memb_hip_pool_rows_device'
        if typed:
            assert call(BAD_OUT_TYPE, MEAN, FAKE) == (INVALID, UNKNOWN_OUT_TYPE), name
            assert call(-1, SUM, FAKE) == (INVALID, 'unknown out_type -1'), name
        assert call(F32, BAD_MODE, FAKE) == (INVALID, UNKNOWN_MODE), name
        assert call(F32, -1, FAKE) == (INVALID, 'unknown pooling mode -1'), name
        assert call(F32, MEAN, None) == (INVALID, NULL_ARGUMENT), name
        if typed:
            assert call(BF16, SUM, None) == (INVALID, NULL_ARGUMENT), name


def test_the_earlier_check_wins(entry_points):
    # out_type before mode before null arguments, at every entry point
    _, calls = entry_points
    for name, call in calls.items():
        if name != 'memb_hip_pool_rows_device':
            assert call(BAD_OUT_TYPE, BAD_MODE, FAKE) == (INVALID, UNKNOWN_OUT_TYPE), name
            assert call(BAD_OUT_TYPE, MEAN, None) == (INVALID, UNKNOWN_OUT_TYPE), name
            assert call(BAD_OUT_TYPE, BAD_MODE, None) == (INVALID, UNKNOWN_OUT_TYPE), name
        assert call(F32, BAD_MODE, None) == (INVALID, UNKNOWN_MODE), name


def test_null_arguments_of_each_entry_point(entry_points):
    # every pointer an entry point needs, missing in turn; none is needed for what is empty (n == 0: rows; bags == 0:
    # offsets and out -- checked with the dense call below, which needs no context to go on)
    library, _ = entry_points

    def refused(code):
        return (code, library.memb_hip_last_error().decode()) == (INVALID, NULL_ARGUMENT)

    for context, rows, offsets, out in ((None, FAKE, FAKE, FAKE), (FAKE, None, FAKE, FAKE), (FAKE, FAKE, None, FAKE),
                                        (FAKE, FAKE, FAKE, None)):
        assert refused(library.memb_hip_pool_rows_device(context, rows, 4, offsets, 1, out, 8, 0, MEAN, None))
        assert refused(library.memb_hip_pool_rows_device_typed(context, rows, 4, offsets, 1, out, F32, 8, 0, MEAN, None))
        assert refused(library.memb_hip_pool_known_rows_device_typed(context, rows, 4, offsets, 1, out, F32, 8, 0, MEAN, None, None))
        assert refused(library.memb_hip_pool_rows_chunked_device_typed(
            context, rows, 4, offsets, 1, out, F32, 8, 0, MEAN, 0, None, FAKE, 1 << 20, None))
    pair = (P * 2)(FAKE, FAKE)
    for contexts, rows, count in ((None, pair, 2), (pair, None, 2), (pair, pair, 0), ((P * 2)(FAKE, None), pair, 2),
                                  (pair, (P * 2)(FAKE, None), 2)):
        assert refused(library.memb_hip_pool_rows_union_device(contexts, rows, count, 4, FAKE, 1, FAKE, F32, 8, 0, MEAN, None))
    assert refused(library.memb_hip_pool_rows_union_device(pair, pair, 2, 4, None, 1, FAKE, F32, 8, 0, MEAN, None))
    assert refused(library.memb_hip_pool_rows_union_device(pair, pair, 2, 4, FAKE, 1, None, F32, 8, 0, MEAN, None))
    for values, offsets, out in ((None, FAKE, FAKE), (FAKE, None, FAKE), (FAKE, FAKE, None)):
        assert refused(library.memb_hip_pool_dense_rows_device(0, values, 4, 8, 8, offsets, 1, out, F32, 8, 0, MEAN, None))


def test_the_dense_call_checks_on_without_a_context(entry_points):
    library, _ = entry_points

    def dense(values=FAKE, n=4, dim=8, ld_values=8, offsets=FAKE, bags=1, out=FAKE, out_type=F32, ld=8, col_off=0, mode=MEAN,
              device=0):
        code = library.memb_hip_pool_dense_rows_device(device, values, n, dim, ld_values, offsets, bags, out, out_type, ld, col_off,
                                                       mode, None)
        return code, library.memb_hip_last_error().decode()

    # its own mistakes, each alone
    assert dense(dim=0, ld_values=0) == (INVALID, DENSE_DIM)
    assert dense(dim=1 << 32, ld_values=1 << 32, ld=1 << 32) == (INVALID, DENSE_DIM)
    assert dense(ld_values=7) == (INVALID, DENSE_DIM)
    assert dense(device=-1) == (INVALID, DENSE_DIM)
    assert dense(out=FAKE + 2) == (INVALID, DENSE_UNALIGNED)                   # fp32 at an odd half
    assert dense(out=FAKE + 1, out_type=BF16) == (INVALID, DENSE_UNALIGNED)
    assert dense(values=FAKE + 2) == (INVALID, DENSE_UNALIGNED)
    assert dense(ld=7) == (INVALID, LD_TOO_SMALL)
    assert dense(ld=8, col_off=1) == (INVALID, LD_TOO_SMALL)
    assert dense(ld=4, col_off=5) == (INVALID, LD_TOO_SMALL)                   # (col_off beyond ld: no wrap-around)
    # in their order: null arguments, dim, alignment, ld -- and all of them before "nothing to do"
    assert dense(offsets=None, dim=0) == (INVALID, NULL_ARGUMENT)
    assert dense(mode=BAD_MODE, dim=0) == (INVALID, UNKNOWN_MODE)
    assert dense(dim=0, out=FAKE + 2, ld=0) == (INVALID, DENSE_DIM)
    assert dense(out=FAKE + 2, ld=7) == (INVALID, DENSE_UNALIGNED)
    assert dense(bags=0, ld=7) == (INVALID, LD_TOO_SMALL)
    assert dense(bags=0, out=FAKE + 2) == (INVALID, DENSE_UNALIGNED)
    assert dense(bags=0, dim=0) == (INVALID, DENSE_DIM)
    assert dense(bags=0, out_type=BAD_OUT_TYPE) == (INVALID, UNKNOWN_OUT_TYPE)
    # bags == 0: MEMB_HIP_OK with nothing launched -- no device is opened (there may be none, and `device` need not exist),
    # no pointer is needed, and with a device nothing could run on these pointers and end well
    assert dense(bags=0)[0] == OK
    assert dense(bags=0, offsets=None, out=None)[0] == OK
    assert dense(bags=0, n=0, values=None, offsets=None, out=None, device=1 << 20)[0] == OK
    assert dense(bags=0, out_type=BF16, mode=SUM)[0] == OK
