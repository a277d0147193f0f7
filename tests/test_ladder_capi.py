"""Ladder calls (include/ulc_amd.h, ulcx_encode_*_ladder) at the C-ABI boundary, without a GPU: the rung's layout, the
exported symbols and their binding, argument checks that need no device, and the command line's refusal of malformed
ladders during argument parsing."""
import ctypes as C
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
LIB = os.path.join(ROOT, "ulc-codec_amd", "libulc_amd.so")
TOOL = os.path.join(ROOT, "ulc-codec_amd", "ulcx-tool")
NAMES = ("ulcx_encode_dev_ladder", "ulcx_encode_dev_pcm16_ladder", "ulcx_encode_host_ladder", "ulcx_encoder_last_rungs")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ulc-codec_amd"), "-j8"], stdout=subprocess.DEVNULL)
    return C.CDLL(LIB)


def test_rung_is_24_bytes_with_the_table_at_16_for_the_c_compiler():
    src = ('#include <stddef.h>\n#include "ulc_amd.h"\n_Static_assert(sizeof(ulcx_rung)==24,"size");\n'
           '_Static_assert(offsetof(ulcx_rung,mode)==0,"m");\n_Static_assert(offsetof(ulcx_rung,param0)==4,"p0");\n'
           '_Static_assert(offsetof(ulcx_rung,param1)==8,"p1");\n_Static_assert(offsetof(ulcx_rung,reserved)==12,"r");\n'
           '_Static_assert(offsetof(ulcx_rung,rate)==16,"t");\n_Static_assert(ULCX_MAX_RUNGS==8,"max");\n'
           'int main(void){return 0;}\n')
    p = subprocess.run(["gcc", "-x", "c", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-"], input=src.encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()
    import ulc_amd
    assert C.sizeof(ulc_amd.Rung) == 24 and ulc_amd.Rung.rate.offset == 16 and ulc_amd.MAX_RUNGS == 8


def test_ladder_entry_points_are_exported_and_bound(lib):
    import ulc_amd
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in ulc_amd.EXPORTS, n
    for m in ("encode_ladder", "encode_dev_ladder", "last_rungs"):
        assert hasattr(ulc_amd.BatchEncoder, m), m


def test_null_encoder_or_null_rungs_is_refused(lib):
    import ulc_amd
    rungs = (ulc_amd.Rung * 2)()
    rungs[0].mode, rungs[0].param0 = 0, 50.0
    rungs[1].mode, rungs[1].param0 = 1, 64.0
    live = C.c_void_p(16)               # (never dereferenced: the rung array is checked first)
    pcm = (C.c_float * 16)()
    out = (C.c_uint8 * 16)()
    bits = (C.c_int32 * 4)()
    for fn in (lib.ulcx_encode_dev_ladder, lib.ulcx_encode_dev_pcm16_ladder):
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 5
        assert fn(None, C.addressof(rungs), 2, C.addressof(pcm), 1, C.addressof(out), C.addressof(bits), None, None, None) == -1
        assert fn(live, None, 2, C.addressof(pcm), 1, C.addressof(out), C.addressof(bits), None, None, None) == -1
    fn = lib.ulcx_encode_host_ladder
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 4
    assert fn(None, C.addressof(rungs), 2, C.addressof(pcm), 1, C.addressof(out), C.addressof(bits), None, None) == -1
    assert fn(live, None, 2, C.addressof(pcm), 1, C.addressof(out), C.addressof(bits), None, None) == -1
    lib.ulcx_encoder_last_rungs.argtypes = [C.c_void_p]
    assert lib.ulcx_encoder_last_rungs(None) == -1


@pytest.mark.skipif(not os.path.exists(TOOL), reason="ulcx-tool not built")
@pytest.mark.parametrize("args,named", [
    (["-50/", "a.wav"], "-50/"), (["/64", "a.wav"], "/64"), (["-50//64", "a.wav"], "-50//64"),
    (["-10/-20/-30/-40/-50/-60/-70/-80/-90", "a.wav"], "-10/-20/-30/-40/-50/-60/-70/-80/-90"),
    (["-50/64", "a.wav", "-rate:48", "b.wav"], "-rate:48"), (["-50", "a.wav", "-rate:48/64", "b.wav"], "-rate:48/64"),
    (["-50/64", "-rate:48/", "a.wav"], "-rate:48/"),
])
def test_cli_refuses_malformed_ladders_while_parsing(tmp_path, args, named):
    """Exit status 2 and a message naming the argument, before any input is opened or any device is asked for (the inputs
    do not exist, and this runs without a GPU)."""
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "ulc-codec_amd") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    p = subprocess.run([TOOL, "encode", str(tmp_path)] + args, capture_output=True, env=env, timeout=60)
    assert p.returncode == 2, p.stderr.decode()
    assert f"'{named}'" in p.stderr.decode(), p.stderr.decode()
    assert os.listdir(tmp_path) == []
