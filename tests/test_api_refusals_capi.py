"""Refusals at the C-ABI boundary, without a GPU (include/ulc_amd.h: "negative return + ulcx_last_error()"): every entry that
takes an encoder or a decoder and returns a status refuses a NULL object with ULCX_ERR_ARG and a message that begins with its
OWN name - not the name of the body it shares with its siblings, and not the text an earlier call left behind.

The entries come from the header itself, so one declared later is covered the day it is declared.

At the parent of the commit that added this file 23 of the 57 entries failed it.
  No message (the text of the call before was still there): ulcx_encoder_reset, ulcx_decoder_reset, ulcx_encode_host,
    ulcx_decode_host, ulcx_decode_packed_host, ulcx_decoder_upload_payload, ulcx_decode_resident_host,
    ulcx_encoder_debug_fetch, ulcx_encoder_debug_force_exact, ulcx_encoder_last_fallbacks, ulcx_encoder_last_rungs,
    ulcx_decoder_last_cut, ulcx_encoder_set_timing, ulcx_decoder_set_timing.
  The name of the entry whose body it shares: ulcx_encode_dev_pcm16, ulcx_encode_dev_rates, ulcx_encode_dev_pcm16_rates,
    ulcx_encode_dev_pcm16_ladder, ulcx_analyse_dev_pcm16, ulcx_decode_dev_pcm16, ulcx_decode_block1_rng,
    ulcx_decode_range_dev, ulcx_decode_range_dev_pcm16."""
import ctypes as C
import os
import re
import subprocess
import sys
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
HEADER = os.path.join(ROOT, "include", "ulc_amd.h")

# object-taking entries that return a count or a size, not a status (0 for no object, by their declarations)
NOT_A_STATUS = {"ulcx_encoder_stage_ms", "ulcx_decoder_stage_ms", "ulcx_encoder_slot_bytes", "ulcx_encoder_last_xf_launches"}


def _ctype(param):
    """ctypes type of one parameter of a declaration, and the "valid-looking" value the first call passes for it"""
    p = re.sub(r"/\*.*?\*/", " ", param).strip()
    if "*" in p or "[" in p:
        return C.c_void_p, "hipStream" not in p            # host memory, but no stream
    if re.match(r"(const\s+)?float\b", p):
        return C.c_float, 50.0
    if re.match(r"(const\s+)?long long\b", p):
        return C.c_longlong, 1
    if re.match(r"(const\s+)?size_t\b", p):
        return C.c_size_t, 1
    assert re.match(r"(const\s+)?int\b", p), param
    return C.c_int, 1


def _entries():
    """{name: [(ctype, value)]} of every `int ulcx_*(ulcx_encoder * | ulcx_decoder *, ...)` the header declares"""
    text = re.sub(r"/\*.*?\*/", " ", open(HEADER).read(), flags=re.S)
    out = {}
    for m in re.finditer(r"\bint\s+(ulcx_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        name, params = m.group(1), [q.strip() for q in m.group(2).split(",")]
        if re.match(r"(const\s+)?ulcx_(encoder|decoder)\s*\*\s*\w+$", params[0]):
            out[name] = [_ctype(q) for q in params[1:]]
    return out


ENTRIES = _entries()
COVERED = sorted(set(ENTRIES) - NOT_A_STATUS)


@pytest.fixture(scope="module")
def lib():
    import ulc_amd
    if not os.path.exists(ulc_amd.LIB_PATH):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ulc-codec_amd"), "-j8"], stdout=subprocess.DEVNULL)
    l = C.CDLL(ulc_amd.LIB_PATH)
    l.ulcx_last_error.restype = C.c_char_p
    l.ulcx_ulc_header_parse.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    return l


def test_the_header_was_understood():
    """The parse finds the entries it should (a few of each family named here), and the ones left out exist and are left out
    for the reason given: they take an object and return an int that is not a status."""
    assert NOT_A_STATUS <= set(ENTRIES), NOT_A_STATUS - set(ENTRIES)
    for n in ("ulcx_encode_dev", "ulcx_encode_host_ladder", "ulcx_analyse_dev_pcm16", "ulcx_encode_block1", "ulcx_decode_block1_rng",
              "ulcx_decode_range_dev_pcm16", "ulcx_decode_resident_range_host", "ulcx_decoder_upload_payload", "ulcx_decoder_last_cut",
              "ulcx_encoder_set_timing", "ulcx_decoder_set_timing", "ulcx_encoder_debug_force_exact", "ulcx_encoder_reset",
              "ulcx_decoder_load_streams_host", "ulcx_index_packed_dev", "ulcx_encoder_debug_writer_flags", "ulcx_encoder_debug_writer_plan"):
        assert n in COVERED, n
    assert len(COVERED) >= 57, len(COVERED)
    assert not [n for n in ENTRIES if "create" in n or "destroy" in n or "stage_name" in n or "state_bytes" in n]


@pytest.mark.parametrize("name", COVERED)
def test_null_object_is_refused_by_name(lib, name):
    buf = (C.c_uint8 * 4096)()
    hdr = (C.c_uint8 * 24)()
    fn = getattr(lib, name)
    fn.restype = C.c_int
    fn.argtypes = [C.c_void_p] + [t for t, _ in ENTRIES[name]]
    looks_valid = [None] + [(C.addressof(buf) if v else None) if t is C.c_void_p else v for t, v in ENTRIES[name]]
    all_null = [None] + [None if t is C.c_void_p else t(0).value for t, _ in ENTRIES[name]]
    for what, args in (("valid-looking arguments", looks_valid), ("all-null arguments", all_null)):
        assert lib.ulcx_ulc_header_parse(C.addressof(hdr), C.addressof(buf), 0) == -1
        assert b"need 24 bytes" in lib.ulcx_last_error()
        assert fn(*args) == -1, (name, what)
        msg = lib.ulcx_last_error().decode()
        assert msg.startswith(name + ":"), (name, what, msg)
