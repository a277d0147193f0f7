"""The analysis-only call (include/ulc_amd.h: ulcx_analyse_dev / _dev_pcm16 / _host) at the C-ABI boundary, without a GPU:
exported symbols and their binding, argument checks that need no device, the header as C, and the tool's sub-command."""
import ctypes as C
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
LIB = os.path.join(ROOT, "ulc-codec_amd", "libulc_amd.so")
TOOL = os.path.join(ROOT, "ulc-codec_amd", "ulcx-tool")
NAMES = ("ulcx_analyse_dev", "ulcx_analyse_dev_pcm16", "ulcx_analyse_host")


@pytest.fixture(scope="module")
def lib():
    if not (os.path.exists(LIB) and os.path.exists(TOOL)):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ulc-codec_amd"), "-j8"], stdout=subprocess.DEVNULL)
    return C.CDLL(LIB)


def test_analysis_entry_points_are_exported_and_bound(lib):
    import ulc_amd
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in ulc_amd.EXPORTS, n
    assert hasattr(ulc_amd.BatchEncoder, "analyse") and hasattr(ulc_amd.BatchEncoder, "analyse_dev")


def test_null_encoder_is_refused(lib):
    pcm = (C.c_float * 16)()
    wc = (C.c_int32 * 4)()
    cplx = (C.c_float * 4)()
    for name in NAMES[:2]:
        fn = getattr(lib, name)
        fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        assert fn(None, C.addressof(pcm), 1, C.addressof(wc), C.addressof(cplx), None) == -1
        assert fn(None, None, 1, C.addressof(wc), C.addressof(cplx), None) == -1
        assert fn(None, C.addressof(pcm), 1, None, None, None) == -1
    fn = lib.ulcx_analyse_host
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert fn(None, C.addressof(pcm), 1, C.addressof(wc), C.addressof(cplx)) == -1
    assert fn(None, None, 1, None, None) == -1


def test_header_compiles_as_c_and_declares_the_calls():
    src = ('#include "ulc_amd.h"\n'
           'int (*a)(ulcx_encoder *, const float *, int, int32_t *, float *, void *) = ulcx_analyse_dev;\n'
           'int (*b)(ulcx_encoder *, const int16_t *, int, int32_t *, float *, void *) = ulcx_analyse_dev_pcm16;\n'
           'int (*c)(ulcx_encoder *, const float *, int, int32_t *, float *) = ulcx_analyse_host;\n'
           'int main(void){return 0;}\n')
    p = subprocess.run(["gcc", "-x", "c", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-"],
                       input=src.encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()


def _tool(args, cwd):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "ulc-codec_amd") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run([TOOL] + args, capture_output=True, env=env, cwd=cwd, timeout=120)


def test_tool_usage_names_the_analyse_sub_command(lib, tmp_path):
    p = _tool([], str(tmp_path))
    assert p.returncode == 1
    assert "ulcx-tool analyse" in p.stderr.decode()
    assert "ulcx-tool encode" in p.stderr.decode() and "ulcx-tool decode" in p.stderr.decode()


def test_tool_analyse_without_a_device_fails_and_writes_nothing(lib, tmp_path):
    """Without a device run_groups refuses before any file is opened (with one, the missing input is refused)."""
    p = _tool(["analyse", "x.wav"], str(tmp_path))
    assert p.returncode != 0
    assert p.stdout == b""
    assert os.listdir(str(tmp_path)) == []


def test_tool_analyse_refuses_bad_options_before_any_device_work(lib, tmp_path):
    for args in (["analyse"], ["analyse", "-blocksize:1000", "x.wav"], ["analyse", "-devices:0", "x.wav"], ["analyse", "-bogus", "x.wav"]):
        p = _tool(args, str(tmp_path))
        assert p.returncode == 2, args
    assert os.listdir(str(tmp_path)) == []
