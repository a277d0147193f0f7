"""Block index and range decode (include/ulc_amd.h section 3: ulcx_index_packed_* / ulcx_decode_range_* and the resident
forms) at the C-ABI boundary, without a GPU: exported symbols and their binding, the header as C, argument checks that need
no device, and the front-end's -blocks: option."""
import ctypes as C
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
LIB = os.path.join(ROOT, "ulc-codec_amd", "libulc_amd.so")
TOOL = os.path.join(ROOT, "ulc-codec_amd", "ulcx-tool")
NAMES = ("ulcx_index_packed_dev", "ulcx_index_packed_host", "ulcx_decode_range_dev", "ulcx_decode_range_dev_pcm16",
         "ulcx_decode_range_host", "ulcx_decoder_index_resident", "ulcx_decode_resident_range_host")
ERR_ARG = -1
P, I, LL = C.c_void_p, C.c_int, C.c_longlong


@pytest.fixture(scope="module")
def lib():
    if not (os.path.exists(LIB) and os.path.exists(TOOL)):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ulc-codec_amd"), "-j8"], stdout=subprocess.DEVNULL)
    return C.CDLL(LIB)


def test_seek_entry_points_are_exported_and_bound(lib):
    import ulc_amd
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in ulc_amd.EXPORTS, n
    for m in ("index_packed", "decode_range", "index_resident", "decode_resident_range"):
        assert hasattr(ulc_amd.BatchDecoder, m), m
    assert ulc_amd.INDEX_DTYPE.itemsize == 8


def test_header_compiles_as_c_and_declares_the_calls():
    src = ('#include "ulc_amd.h"\n'
           '_Static_assert(sizeof(ulcx_index_entry) == 8, "");\n'
           'int (*a)(ulcx_decoder *, const uint8_t *, long long, const int32_t *, int, ulcx_index_entry *, int32_t *, void *) = ulcx_index_packed_dev;\n'
           'int (*b)(ulcx_decoder *, const uint8_t *, long long, const int32_t *, int, ulcx_index_entry *, int32_t *) = ulcx_index_packed_host;\n'
           'int (*c)(ulcx_decoder *, const uint8_t *, long long, const int32_t *, const ulcx_index_entry *, int, const int32_t *,\n'
           '         const int32_t *, int, float *, int32_t *, void *) = ulcx_decode_range_dev;\n'
           'int (*d)(ulcx_decoder *, const uint8_t *, long long, const int32_t *, const ulcx_index_entry *, int, const int32_t *,\n'
           '         const int32_t *, int, int16_t *, int32_t *, void *) = ulcx_decode_range_dev_pcm16;\n'
           'int (*e)(ulcx_decoder *, const uint8_t *, long long, const int32_t *, const ulcx_index_entry *, int, const int32_t *,\n'
           '         const int32_t *, int, float *, int32_t *) = ulcx_decode_range_host;\n'
           'int (*f)(ulcx_decoder *, int, int32_t *) = ulcx_decoder_index_resident;\n'
           'int (*g)(ulcx_decoder *, const int32_t *, int, float *, int32_t *) = ulcx_decode_resident_range_host;\n'
           'ulcx_index_entry en = { -1, 0u };\n'
           'int main(void){return en.ByteOffs + (int)en.RngState;}\n')
    p = subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-"],
                       input=src.encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()


def test_bad_arguments_are_refused_without_a_device(lib):
    """A NULL decoder, maxBlocks < 1 and nBlocks < 1: ULCX_ERR_ARG from every form, before anything touches a device."""
    buf = (C.c_uint8 * 64)()
    n = (C.c_int32 * 4)()
    idx = (C.c_uint8 * 64)()
    pcm = (C.c_float * 16)()
    b, nn, ix, pc = C.addressof(buf), C.addressof(n), C.addressof(idx), C.addressof(pcm)
    lib.ulcx_index_packed_dev.argtypes = [P, P, LL, P, I, P, P, P]
    lib.ulcx_index_packed_host.argtypes = [P, P, LL, P, I, P, P]
    for mb in (4, 0, -3):
        assert lib.ulcx_index_packed_dev(None, b, 64, nn, mb, ix, nn, None) == ERR_ARG
        assert lib.ulcx_index_packed_host(None, b, 64, nn, mb, ix, nn) == ERR_ARG
    rng = [P, P, LL, P, P, I, P, P, I, P, P]
    lib.ulcx_decode_range_dev.argtypes = rng + [P]
    lib.ulcx_decode_range_dev_pcm16.argtypes = rng + [P]
    lib.ulcx_decode_range_host.argtypes = rng
    for nb in (2, 0, -1):
        assert lib.ulcx_decode_range_dev(None, b, 64, nn, ix, 5, nn, nn, nb, pc, nn, None) == ERR_ARG
        assert lib.ulcx_decode_range_dev_pcm16(None, b, 64, nn, ix, 5, nn, nn, nb, pc, nn, None) == ERR_ARG
        assert lib.ulcx_decode_range_host(None, b, 64, nn, ix, 5, nn, nn, nb, pc, nn) == ERR_ARG
    lib.ulcx_decoder_index_resident.argtypes = [P, I, P]
    lib.ulcx_decode_resident_range_host.argtypes = [P, P, I, P, P]
    for mb in (4, 0):
        assert lib.ulcx_decoder_index_resident(None, mb, nn) == ERR_ARG
    for nb in (2, 0):
        assert lib.ulcx_decode_resident_range_host(None, nn, nb, pc, nn) == ERR_ARG


def test_range_tail_plan_arithmetic(lib):
    """ulcx_dec_range_tail_plan: calls of 24 blocks or more as ulcx_dec_tail_plan; shorter ones (6 or more, more streams than
    the device holds) in pieces of max(2, nBlocks / 4) blocks; nothing when the last round is empty or more than 4/5 full."""
    f, g = C.c_int32(-1), C.c_int32(-1)
    plan = lambda *a: (lib.ulcx_dec_range_tail_plan(*a, C.byref(f)), f.value)
    for shape in ((4096, 31, 1536), (2560, 24, 1536), (4096, 32, 1536), (1000, 26, 1536), (3072, 40, 1536)):
        assert plan(*shape) == (lib.ulcx_dec_tail_plan(*shape, C.byref(g)), g.value), shape
    assert plan(1600, 7, 1536) == (64 * 7 // 2, 1536)
    assert plan(1600, 16, 1536) == (64 * 16 // 4, 1536)
    assert plan(1600, 5, 1536) == (0, 0)                    # fewer than three pieces of two blocks
    assert plan(1536, 7, 1536) == (0, 0) and plan(3072, 7, 1536) == (0, 0)      # whole rounds only
    assert plan(1000, 7, 1536) == (0, 0)                    # no whole round in front of the last one
    assert plan(3000, 7, 1536) == (0, 0)                    # last round 95 % full
    assert plan(0, 7, 1536) == (0, 0) and plan(1600, 7, 0) == (0, 0)
    import ulc_amd
    assert "ulcx_dec_range_tail_plan" in ulc_amd.EXPORTS


def _tool(args, cwd):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "ulc-codec_amd") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run([TOOL] + args, capture_output=True, env=env, cwd=cwd, timeout=120)


def test_tool_usage_names_the_blocks_option(lib, tmp_path):
    p = _tool([], str(tmp_path))
    assert p.returncode == 1
    assert "-blocks:" in p.stderr.decode()


@pytest.mark.parametrize("value", ["x", "-1,4", "3,0", "3", "3,", ",3", "1,2x", "1.5,2"])
def test_tool_refuses_a_malformed_block_range_before_any_device_work(lib, tmp_path, value):
    out = tmp_path / "out"
    out.mkdir()
    p = _tool(["decode", str(out), f"-blocks:{value}", "x.ulc"], str(tmp_path))
    assert p.returncode == 2, (value, p.stderr.decode())
    assert "block range" in p.stderr.decode()
    assert os.listdir(str(out)) == []
