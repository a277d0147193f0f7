"""Per-stream rate settings (include/ulc_amd.h, ulcx_encode_*_rates) at the C-ABI boundary, without a GPU: the table
entry's layout, the exported symbols and their binding, argument checks that need no device, and the per-block oracle
driver the GPU tests compare against (tests/rates_testlib.py)."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
LIB = os.path.join(ROOT, "ulc-codec_amd", "libulc_amd.so")
NAMES = ("ulcx_encode_dev_rates", "ulcx_encode_dev_pcm16_rates", "ulcx_encode_host_rates")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ulc-codec_amd"), "-j8"], stdout=subprocess.DEVNULL)
    return C.CDLL(LIB)


def test_rate_entry_is_eight_bytes_for_the_c_compiler():
    src = ('#include <stddef.h>\n#include "ulc_amd.h"\n_Static_assert(sizeof(ulcx_rate)==8,"size");\n'
           '_Static_assert(offsetof(ulcx_rate,RateKbps)==0,"r");\n_Static_assert(offsetof(ulcx_rate,AvgComplexity)==4,"a");\n'
           'int main(void){return 0;}\n')
    p = subprocess.run(["gcc", "-x", "c", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-"], input=src.encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()


def test_rate_entry_points_are_exported_and_bound(lib):
    import ulc_amd
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in ulc_amd.EXPORTS, n
    assert hasattr(ulc_amd.BatchEncoder, "encode_rates") and hasattr(ulc_amd.BatchEncoder, "encode_dev_rates")


def test_null_encoder_or_null_table_is_refused(lib):
    table = (C.c_float * 2)(64.0, 0.0)
    pcm = (C.c_float * 16)()
    out = (C.c_uint8 * 16)()
    bits = (C.c_int32 * 4)()
    for fn in (lib.ulcx_encode_dev_rates, lib.ulcx_encode_dev_pcm16_rates):
        fn.argtypes = [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 5
        assert fn(None, C.addressof(table), C.addressof(pcm), 1, C.addressof(out), C.addressof(bits), None, None, None) == -1
        assert fn(None, None, C.addressof(pcm), 1, C.addressof(out), C.addressof(bits), None, None, None) == -1
    fn = lib.ulcx_encode_host_rates
    fn.argtypes = [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 4
    assert fn(None, C.addressof(table), C.addressof(pcm), 1, C.addressof(out), C.addressof(bits), None, None) == -1
    assert fn(None, None, C.addressof(pcm), 1, C.addressof(out), C.addressof(bits), None, None) == -1


@pytest.mark.parametrize("setting,mode,p0,p1", [((-50.0, 0.0), 0, 50.0, 0.0), ((64.0, 0.0), 1, 64.0, 0.0), ((96.0, 0.41), 2, 96.0, 0.41),
                                                 ((-50.0, 0.3), 0, 50.0, 0.0)])
def test_per_block_oracle_driver_matches_the_whole_stream_oracle(setting, mode, p0, p1):
    """The driver the GPU tests use (one orc_encoder per stream, block by block) equals orc_encode_stream_debug for a
    fixed setting, and reads a setting as ulcEncodeTool.c:157-159 does (a negative rate is VBR whatever the complexity)."""
    from ulc_testlib import synth_pcm, oracle_encode_debug
    from rates_testlib import oracle_streams, mode_of
    assert mode_of(setting)[0] == mode
    bs, ch, rate, K = 1024, 2, 44100, 5
    pcm = synth_pcm(7, K * bs, ch, rate, transient=True, seed=3)
    got = oracle_streams(pcm[None], bs, rate, [[setting]])[0]
    ref = oracle_encode_debug(pcm, bs, rate, mode, p0, np.float32(p1))
    for k in range(K):
        assert got[k]["bits"] == ref["bits"][k] and got[k]["wc"] == ref["wc"][k] and got[k]["nout"] == ref["nout"][k]
        assert np.array_equal(got[k]["bytes"], ref["out"][k, :ref["bits"][k] // 8])
        assert np.array_equal(got[k]["keep"], (ref["ranks"][k] < ref["nout"][k]).astype(np.uint8))
