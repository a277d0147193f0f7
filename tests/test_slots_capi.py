"""Stream slots (include/ulc_amd.h: per-stream reset, save / load, subset calls) at the C-ABI boundary, without a GPU:
exported symbols, their declarations as C, the binding, and the argument checks that need no device."""
import ctypes as C
import os
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
LIB = os.path.join(ROOT, "ulc-codec_amd", "libulc_amd.so")

V, I, F = C.c_void_p, C.c_int, C.c_float
# name -> (C declaration of a pointer to it, ctypes argument types)
ENTRIES = {
    "ulcx_encoder_reset_streams_dev": ("int (*%s)(ulcx_encoder *, const int32_t *, int, void *)", [V, V, I, V]),
    "ulcx_encoder_save_streams_dev": ("int (*%s)(ulcx_encoder *, const int32_t *, int, uint8_t *, void *)", [V, V, I, V, V]),
    "ulcx_encoder_load_streams_dev": ("int (*%s)(ulcx_encoder *, const int32_t *, int, const uint8_t *, void *)", [V, V, I, V, V]),
    "ulcx_decoder_reset_streams_dev": ("int (*%s)(ulcx_decoder *, const int32_t *, int, void *)", [V, V, I, V]),
    "ulcx_decoder_save_streams_dev": ("int (*%s)(ulcx_decoder *, const int32_t *, int, uint8_t *, void *)", [V, V, I, V, V]),
    "ulcx_decoder_load_streams_dev": ("int (*%s)(ulcx_decoder *, const int32_t *, int, const uint8_t *, void *)", [V, V, I, V, V]),
    "ulcx_encoder_reset_streams_host": ("int (*%s)(ulcx_encoder *, const int32_t *, int)", [V, V, I]),
    "ulcx_encoder_save_streams_host": ("int (*%s)(ulcx_encoder *, const int32_t *, int, uint8_t *)", [V, V, I, V]),
    "ulcx_encoder_load_streams_host": ("int (*%s)(ulcx_encoder *, const int32_t *, int, const uint8_t *)", [V, V, I, V]),
    "ulcx_decoder_reset_streams_host": ("int (*%s)(ulcx_decoder *, const int32_t *, int)", [V, V, I]),
    "ulcx_decoder_save_streams_host": ("int (*%s)(ulcx_decoder *, const int32_t *, int, uint8_t *)", [V, V, I, V]),
    "ulcx_decoder_load_streams_host": ("int (*%s)(ulcx_decoder *, const int32_t *, int, const uint8_t *)", [V, V, I, V]),
    "ulcx_encode_dev_subset": ("int (*%s)(ulcx_encoder *, const int32_t *, int, int, float, float, const ulcx_rate *, const float *, int, "
                               "uint8_t *, int32_t *, int32_t *, float *, void *)", [V, V, I, I, F, F, V, V, I, V, V, V, V, V]),
    "ulcx_encode_dev_pcm16_subset": ("int (*%s)(ulcx_encoder *, const int32_t *, int, int, float, float, const ulcx_rate *, const int16_t *, int, "
                                     "uint8_t *, int32_t *, int32_t *, float *, void *)", [V, V, I, I, F, F, V, V, I, V, V, V, V, V]),
    "ulcx_analyse_dev_subset": ("int (*%s)(ulcx_encoder *, const int32_t *, int, const float *, int, int32_t *, float *, void *)",
                                [V, V, I, V, I, V, V, V]),
    "ulcx_encode_host_subset": ("int (*%s)(ulcx_encoder *, const int32_t *, int, int, float, float, const ulcx_rate *, const float *, int, "
                                "uint8_t *, int32_t *, int32_t *, float *)", [V, V, I, I, F, F, V, V, I, V, V, V, V]),
    "ulcx_decode_dev_subset": ("int (*%s)(ulcx_decoder *, const int32_t *, int, const uint8_t *, int, int, float *, int32_t *, void *)",
                               [V, V, I, V, I, I, V, V, V]),
    "ulcx_decode_dev_pcm16_subset": ("int (*%s)(ulcx_decoder *, const int32_t *, int, const uint8_t *, int, int, int16_t *, int32_t *, void *)",
                                     [V, V, I, V, I, I, V, V, V]),
    "ulcx_decode_host_subset": ("int (*%s)(ulcx_decoder *, const int32_t *, int, const uint8_t *, int, int, float *, int32_t *)",
                                [V, V, I, V, I, I, V, V]),
}
SIZES = {"ulcx_encoder_stream_state_bytes": "size_t (*%s)(const ulcx_encoder *)", "ulcx_decoder_stream_state_bytes": "size_t (*%s)(const ulcx_decoder *)"}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ulc-codec_amd"), "-j8"], stdout=subprocess.DEVNULL)
    return C.CDLL(LIB)


def test_every_slot_entry_is_exported_and_bound(lib):
    import ulc_amd
    for n in list(ENTRIES) + list(SIZES):
        assert hasattr(lib, n), n
        assert n in ulc_amd.EXPORTS, n
    for cls in (ulc_amd.BatchEncoder, ulc_amd.BatchDecoder):
        for m in ("reset_streams", "save_streams", "load_streams", "reset_streams_dev", "save_streams_dev", "load_streams_dev", "state_bytes"):
            assert hasattr(cls, m), (cls.__name__, m)
    for m in ("encode_subset", "encode_subset_dev", "analyse_subset_dev"):
        assert hasattr(ulc_amd.BatchEncoder, m), m
    for m in ("decode_subset", "decode_subset_dev"):
        assert hasattr(ulc_amd.BatchDecoder, m), m


def test_header_compiles_as_c_and_declares_every_entry():
    lines = ['#include "ulc_amd.h"']
    for i, (n, (decl, _)) in enumerate(list(ENTRIES.items()) + [(n, (d, None)) for n, d in SIZES.items()]):
        lines.append((decl % f"p{i}") + f" = {n};")
    lines.append("int main(void){return 0;}")
    p = subprocess.run(["gcc", "-x", "c", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-"],
                       input="\n".join(lines).encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()


def test_null_object_is_refused_by_every_entry(lib):
    """ULCX_ERR_ARG for a NULL object, whatever else is passed (valid-looking host memory: nothing may be touched)."""
    buf = (C.c_uint8 * 4096)()
    slots = (C.c_int32 * 4)(0, 1, 2, 3)
    a, s = C.addressof(buf), C.addressof(slots)
    for name, (_, argtypes) in ENTRIES.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = C.c_int
        args = [None, s]
        for t in argtypes[2:]:
            args.append(1 if t is I else 50.0 if t is F else a)
        if not name.endswith("_host") and "_host_" not in name:
            args[-1] = None                                # hipStream
        assert fn(*args) == -1, name
        nulls = [None] + [0 if t is I else 0.0 if t is F else None for t in argtypes[1:]]
        assert fn(*nulls) == -1, name


def test_state_bytes_of_no_object_is_zero(lib):
    for n in SIZES:
        fn = getattr(lib, n)
        fn.argtypes = [V]
        fn.restype = C.c_size_t
        assert fn(None) == 0, n
