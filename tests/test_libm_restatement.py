"""The product's restatement of glibc expf/logf/log (ulc-codec_amd/csrc/ulcx_libm.h),
compiled for the host, against the live libm of the machine running the tests.
(Full 2^32 sweep: run cmp_expf/cmp_logf with stride 1 — 0 mismatches on glibc 2.35.)"""
import ctypes as C
import numpy as np
import pytest
import units_testlib


@pytest.fixture(scope="module")
def lib():
    return units_testlib.libm_check()                 # builds tests/helpers/libm_check.so when it is older than its sources


@pytest.mark.parametrize("fn", ["cmp_expf", "cmp_logf"])
def test_f32_functions_bit_exact_on_strided_sweep(lib, fn):
    bad = C.c_uint32(0)
    # every 61st bit pattern of the whole binary32 space (~70 M points incl. NaN/inf/subnormals)
    n = getattr(lib, fn)(0, 1 << 32, 61, C.byref(bad))
    assert n == 0, f"{n} mismatches, first at bit pattern {bad.value:#010x}"


def test_f32_functions_dense_near_hot_ranges(lib):
    bad = C.c_uint32(0)
    # expf arguments in the codec are mostly in [-60, 5]; logf arguments are positive ratios
    assert lib.cmp_expf(0xC0000000, 0xC2800000, 1, C.byref(bad)) == 0   # [-2, -64]
    assert lib.cmp_logf(0x3F000000, 0x40000000, 1, C.byref(bad)) == 0   # [0.5, 2)


def test_f64_log_bit_exact_on_random_sample(lib):
    bad = C.c_uint64(0)
    n = lib.cmp_log(0xC0FFEE, 4_000_000, C.byref(bad))
    assert n == 0, f"{n} mismatches, first at {bad.value:#018x}"


def test_array_forms_host_restatement_against_libm(lib):
    """the array entry points the device tests use (tests/test_gpu_units.py), here fed with the HOST compile's results:
    a generated range, an explicit list, and the binary64 inputs of cmp_log"""
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    bad, want = C.c_uint32(0), C.c_uint32(0)
    for fn, grids in ((0, [(0, 1 << 32, 65521), (0xC2CF0000, 0xC2D00000, 1), (0x42B10000, 0x42B20000, 1)]), (1, [(0, 1 << 32, 65521), (0, 0x00010000, 1)])):
        for lo, hi, stride in grids:
            n = (hi - lo + stride - 1) // stride
            got = np.empty(n, np.uint32)
            lib.arr_f32(fn, None, lo, stride, n, p(got))
            assert lib.cmp_f32_arr(fn, p(got), None, lo, stride, n, C.byref(bad), C.byref(want)) == 0, f"fn {fn}: first at {bad.value:#010x}, libm {want.value:#010x}"
            pats = (lo + stride * np.arange(n, dtype=np.uint64)).astype(np.uint32)[::-1].copy()          # the same points as a list, reversed
            lib.arr_f32(fn, p(pats), 0, 0, n, p(got))
            assert lib.cmp_f32_arr(fn, p(got), p(pats), 0, 0, n, C.byref(bad), C.byref(want)) == 0
            i = int(np.flatnonzero(np.isfinite(got.view(np.float32)))[n // 8])                           # a wrong result is found, with its argument
            got[i] ^= 1
            assert lib.cmp_f32_arr(fn, p(got), p(pats), 0, 0, n, C.byref(bad), C.byref(want)) == 1 and bad.value == pats[i]
    x = np.empty(40_000, np.uint64)
    lib.gen_log_inputs(0xC0FFEE, x.size, p(x))
    got = np.empty_like(x)
    lib.arr_log(p(x), x.size, p(got))
    bad64, want64 = C.c_uint64(0), C.c_uint64(0)
    assert lib.cmp_log_arr(p(got), p(x), x.size, C.byref(bad64), C.byref(want64)) == 0, f"log: first at {bad64.value:#018x}"
    got[7] ^= 1
    assert lib.cmp_log_arr(p(got), p(x), x.size, C.byref(bad64), C.byref(want64)) == 1 and bad64.value == x[7]
