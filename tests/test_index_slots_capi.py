"""Index while encoding (include/ulc_amd.h section 3: ulcx_index_begin_dev / ulcx_index_slots_*, ulcx_index_check,
ulcx_decoder_set_resident_index and the `.ulx` sidecar) at the C-ABI boundary, without a GPU: exported symbols and their
binding, the header as C, every refusal that needs no device, the sidecar's header and the host-side index check."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "ulc-codec_amd", "libulc_amd.so")
TOOL = os.path.join(ROOT, "ulc-codec_amd", "ulcx-tool")
NAMES = ("ulcx_index_begin_dev", "ulcx_index_slots_dev", "ulcx_index_slots_host", "ulcx_index_check", "ulcx_decoder_set_resident_index",
         "ulcx_ulx_header_pack", "ulcx_ulx_header_parse")
ERR_ARG = -1
P, I, LL = C.c_void_p, C.c_int, C.c_longlong


@pytest.fixture(scope="module")
def lib():
    if not (os.path.exists(LIB) and os.path.exists(TOOL)):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ulc-codec_amd"), "-j8"], stdout=subprocess.DEVNULL)
    l = C.CDLL(LIB)
    l.ulcx_last_error.restype = C.c_char_p
    l.ulcx_index_begin_dev.argtypes = [P, I, P, I, P, P]
    l.ulcx_index_slots_dev.argtypes = [P, I, P, I, P, I, P, I, P, P]
    l.ulcx_index_slots_host.argtypes = [P, I, P, I, P, I, P, I, P]
    l.ulcx_index_check.argtypes = [P, I, I, LL]
    l.ulcx_decoder_set_resident_index.argtypes = [P, P, I, P]
    return l


def test_entry_points_are_exported_and_bound(lib):
    import ulc_amd
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in ulc_amd.EXPORTS, n
    for m in ("index_begin_dev", "index_slots_dev", "index_slots", "set_resident_index"):
        assert hasattr(ulc_amd.BatchDecoder, m), m
    for f in ("new_index", "index_check", "ulx_pack", "ulx_parse"):
        assert hasattr(ulc_amd, f), f
    assert C.sizeof(ulc_amd.IndexFileHeader) == 16


def test_header_compiles_as_c_and_declares_the_calls():
    src = ('#include "ulc_amd.h"\n'
           '_Static_assert(sizeof(ulcx_index_file_header) == 16 && ULCX_ULX_HEADER_BYTES == 16, "");\n'
           'int (*a)(ulcx_decoder *, int, ulcx_index_entry *, int, int32_t *, void *) = ulcx_index_begin_dev;\n'
           'int (*b)(ulcx_decoder *, int, const uint8_t *, int, const int32_t *, int, ulcx_index_entry *, int, int32_t *, void *) = ulcx_index_slots_dev;\n'
           'int (*c)(ulcx_decoder *, int, const uint8_t *, int, const int32_t *, int, ulcx_index_entry *, int, int32_t *) = ulcx_index_slots_host;\n'
           'int (*d)(const ulcx_index_entry *, int, int, long long) = ulcx_index_check;\n'
           'int (*e)(ulcx_decoder *, const ulcx_index_entry *, int, const int32_t *) = ulcx_decoder_set_resident_index;\n'
           'void (*f)(uint8_t *, const ulcx_index_file_header *) = ulcx_ulx_header_pack;\n'
           'int (*g)(ulcx_index_file_header *, const uint8_t *, size_t) = ulcx_ulx_header_parse;\n'
           'int main(void){return ULCX_ULX_MAGIC == ULCX_ULC_MAGIC;}\n')
    p = subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-"],
                       input=src.encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()


def _bufs():
    slots = (C.c_uint8 * 256)()
    bits = (C.c_int32 * 8)()
    idx = (C.c_int32 * 64)()
    cnt = (C.c_int32 * 8)()
    return slots, bits, idx, cnt, C.addressof(slots), C.addressof(bits), C.addressof(idx), C.addressof(cnt)


def test_bad_arguments_are_refused_without_a_device(lib):
    """Every ULCX_ERR_ARG of the three calls that takes no device to see: the decoder is looked at last, so with a NULL decoder
    the message names the argument that was wrong - or "no decoder" when nothing else is (ULCX_ERR_ARG, not ULCX_ERR_NO_DEVICE:
    nothing has touched a device)."""
    _keep = _bufs()
    s, b, ix, n = _keep[4:]
    err = lambda: lib.ulcx_last_error().decode()
    good = dict(nRows=2, slots=s, slotBytes=32, bits=b, nBlocks=4, index=ix, stride=8, cnt=n)

    def slots_dev(**kw):
        a = dict(good, **kw)
        return lib.ulcx_index_slots_dev(None, a["nRows"], a["slots"], a["slotBytes"], a["bits"], a["nBlocks"], a["index"], a["stride"], a["cnt"], None)

    def slots_host(**kw):
        a = dict(good, **kw)
        return lib.ulcx_index_slots_host(None, a["nRows"], a["slots"], a["slotBytes"], a["bits"], a["nBlocks"], a["index"], a["stride"], a["cnt"])

    def begin(**kw):
        a = dict(good, **kw)
        return lib.ulcx_index_begin_dev(None, a["nRows"], a["index"], a["stride"], a["cnt"], None)

    assert slots_dev() == ERR_ARG and "no decoder" in err()
    assert slots_host() == ERR_ARG and "no decoder" in err()
    assert begin() == ERR_ARG and "no decoder" in err()
    for key in ("slots", "bits", "index", "cnt"):
        assert slots_dev(**{key: None}) == ERR_ARG and "bad argument" in err(), key
        assert slots_host(**{key: None}) == ERR_ARG and "bad argument" in err(), key
    for key in ("index", "cnt"):
        assert begin(**{key: None}) == ERR_ARG and "bad argument" in err(), key
    for key in ("nRows", "nBlocks", "stride", "slotBytes"):
        for v in (0, -3):
            assert slots_dev(**{key: v}) == ERR_ARG and "bad argument" in err(), (key, v)
            assert slots_host(**{key: v}) == ERR_ARG and "bad argument" in err(), (key, v)
    for key in ("nRows", "stride"):
        for v in (0, -3):
            assert begin(**{key: v}) == ERR_ARG and "bad argument" in err(), (key, v)
    # alignment: 4 bytes for d_bits, d_index and d_nBlocks, none for d_slots
    for key, base in (("bits", b), ("index", ix), ("cnt", n)):
        for off in (1, 2, 3):
            assert slots_dev(**{key: base + off}) == ERR_ARG and "not aligned to 4 bytes" in err(), (key, off)
    for key, base in (("index", ix), ("cnt", n)):
        assert begin(**{key: base + 2}) == ERR_ARG and "not aligned to 4 bytes" in err(), key
    assert slots_dev(slots=s + 1) == ERR_ARG and "no decoder" in err()      # an odd slot address passes the argument checks
    # the host form's counts: outside [0, indexStride - 1], before any device work
    cnt = (C.c_int32 * 2)(0, 8)
    assert slots_host(cnt=C.addressof(cnt)) == ERR_ARG and "row 1 counts 8" in err()
    cnt = (C.c_int32 * 2)(-1, 0)
    assert slots_host(cnt=C.addressof(cnt)) == ERR_ARG and "row 0 counts -1" in err()
    cnt = (C.c_int32 * 2)(7, 0)
    assert slots_host(cnt=C.addressof(cnt)) == ERR_ARG and "no decoder" in err()
    assert lib.ulcx_decoder_set_resident_index(None, ix, 8, n) == ERR_ARG


def test_ulx_header_round_trip_short_input_and_bad_magic(lib):
    import ulc_amd
    row = ulc_amd.new_index(1, 5)[0]
    row["ByteOffs"][:4] = [0, 10, 25, 31]
    row["RngState"][1:4] = [7, 0xFFFFFFFF, 9]
    data = ulc_amd.ulx_pack(row, 3, 2048, 2, 31)
    assert len(data) == 16 + 8 * 4
    assert data[:16] == b"ULX1" + bytes([0, 8, 2, 0, 3, 0, 0, 0, 31, 0, 0, 0])             # little-endian, field by field
    h, ent = ulc_amd.ulx_parse(data)
    assert (h.Magic, h.BlockSize, h.nChan, h.nBlocks, h.PayloadBytes) == (0x31584C55, 2048, 2, 3, 31)
    assert np.array_equal(ent, row[:4])
    big = ulc_amd.IndexFileHeader(0x31584C55, 32768, 255, 0xFFFFFFFE, 0x7FFFFFFF)
    hb = (C.c_uint8 * 16)()
    ulc_amd.lib().ulcx_ulx_header_pack(hb, C.byref(big))
    back = ulc_amd.IndexFileHeader()
    assert ulc_amd.lib().ulcx_ulx_header_parse(C.byref(back), hb, 16) == 0
    assert bytes(back) == bytes(big)
    assert ulc_amd.lib().ulcx_ulx_header_parse(C.byref(back), hb, 15) == ERR_ARG                # short
    with pytest.raises(ulc_amd.UlcError):
        ulc_amd.ulx_parse(data[:15])
    with pytest.raises(ulc_amd.UlcError):
        ulc_amd.ulx_parse(data[:-1])                                                            # an entry cut short
    with pytest.raises(ulc_amd.UlcError, match="not a ULX1"):
        ulc_amd.ulx_parse(b"ULC2" + data[4:])                                                   # the container's magic
    with pytest.raises(ulc_amd.UlcError):
        ulc_amd.ulx_parse(b"\0" * 48)


def test_index_check_accepts_the_oracles_walk_and_refuses_each_defect():
    import ulc_amd
    from seek_testlib import geometries, pack, oracle_walk, SEED0
    bs, ch = 512, 1
    _, blocks, bits, _ = geometries()[(bs, ch)][0]
    host, nb = pack([(blocks, bits)])
    K, nbytes = len(bits), int(nb[0])
    wbits, offs, seeds, inside = oracle_walk(host[0], nbytes, ch, bs, K)
    assert len(wbits) == K and inside and seeds[0] == SEED0
    stride = K + 4
    row = ulc_amd.new_index(1, stride)[0]
    row["ByteOffs"][:K + 1] = offs
    row["RngState"][:K + 1] = seeds
    ok = lambda r, n=K, st=stride, pay=nbytes: ulc_amd.index_check(r[:st], n, pay)
    err = lambda: ulc_amd.lib().ulcx_last_error().decode()
    assert ok(row) and ok(row, pay=nbytes + 100) and ok(row, n=K - 3) and ok(row, n=0, pay=0)
    assert ok(row, st=K + 1)                                                # nBlocks = indexStride - 1: the table is full
    bad = row.copy(); bad["ByteOffs"][0] = 1
    assert not ok(bad) and "entry 0" in err()
    bad = row.copy(); bad["RngState"][0] = 0
    assert not ok(bad) and "entry 0" in err()
    for k in (1, 7, K):
        bad = row.copy(); bad["ByteOffs"][k] = bad["ByteOffs"][k - 1]       # an empty block
        assert not ok(bad) and f"entry {k} " in err(), k
        bad = row.copy(); bad["ByteOffs"][k] = bad["ByteOffs"][k - 1] - 1   # going backwards
        assert not ok(bad), k
    bad = row.copy(); bad["ByteOffs"][5] = -1
    assert not ok(bad)
    assert not ok(row, pay=nbytes - 1) and "closes at byte" in err()        # the closing offset past the payload
    assert ok(row, n=K - 1, pay=int(offs[K - 1])) and not ok(row, n=K - 1, pay=int(offs[K - 1]) - 1)
    assert not ok(row, n=-1) and not ok(row, n=stride) and not ok(row, n=stride + 5)      # a bad count
    assert ulc_amd.lib().ulcx_index_check(None, 0, 1, 0) == ERR_ARG


def _tool(args, cwd):
    env = dict(os.environ)
    env["LD_LIBRARY_PATH"] = os.path.join(ROOT, "ulc-codec_amd") + ":/opt/rocm/lib:" + env.get("LD_LIBRARY_PATH", "")
    return subprocess.run([TOOL] + args, capture_output=True, env=env, cwd=cwd, timeout=120)


def test_tool_usage_names_the_index_option(lib, tmp_path):
    p = _tool([], str(tmp_path))
    assert p.returncode == 1
    assert "-index" in p.stderr.decode() and ".ulx" in p.stderr.decode()
