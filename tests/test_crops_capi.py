"""Crops of a resident corpus (include/ulc_amd.h section 3: ulcx_decode_crops_* / ulcx_index_packed_rows_*) at the C-ABI
boundary and ulc-codec_amd/corpus.py's host logic, without a GPU: exported symbols and their binding, the header as C, the
refusals that need no device in their order, `.ulc` / `.ulx` parsing, and the frozen layout on numpy arrays."""
import ctypes as C
import os
import struct
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
LIB = os.path.join(ROOT, "ulc-codec_amd", "libulc_amd.so")
NAMES = ("ulcx_decode_crops_dev", "ulcx_decode_crops_dev_pcm16", "ulcx_decode_crops_host", "ulcx_index_packed_rows_dev",
         "ulcx_index_packed_rows_host")
ERR_ARG = -1
P, I, LL = C.c_void_p, C.c_int, C.c_longlong


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ulc-codec_amd"), "-j8"], stdout=subprocess.DEVNULL)
    l = C.CDLL(LIB)
    l.ulcx_last_error.restype = C.c_char_p
    return l


def test_crop_entry_points_are_exported_and_bound(lib):
    import ulc_amd
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in ulc_amd.EXPORTS, n
    for m in ("decode_crops", "decode_crops_dev", "index_packed_rows", "index_packed_rows_dev"):
        assert hasattr(ulc_amd.BatchDecoder, m), m
    import corpus
    for m in ("add_file", "layout", "freeze", "crops"):
        assert hasattr(corpus.CropCorpus, m), m


def test_header_compiles_as_c_and_declares_the_calls():
    crop = ('ulcx_decoder *, int, const uint8_t *, long long, const int32_t *, const ulcx_index_entry *, int, const int32_t *,\n'
            '         int, const int32_t *, const int32_t *, const int32_t *, int, ')
    src = ('#include "ulc_amd.h"\n'
           f'int (*a)({crop}float *, int32_t *, void *) = ulcx_decode_crops_dev;\n'
           f'int (*b)({crop}int16_t *, int32_t *, void *) = ulcx_decode_crops_dev_pcm16;\n'
           f'int (*c)({crop}float *, int32_t *) = ulcx_decode_crops_host;\n'
           'int (*d)(ulcx_decoder *, int, const uint8_t *, long long, const int32_t *, int, ulcx_index_entry *, int32_t *, void *) = ulcx_index_packed_rows_dev;\n'
           'int (*e)(ulcx_decoder *, int, const uint8_t *, long long, const int32_t *, int, ulcx_index_entry *, int32_t *) = ulcx_index_packed_rows_host;\n'
           'int main(void){return 0;}\n')
    p = subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-"],
                       input=src.encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()


def test_refusals_without_a_device_come_in_order(lib):
    """No object, so every call is refused before anything touches a device; which argument the refusal names shows the order of
    the checks: NULL pointers, n, nFiles, nBlocks - and only then the missing decoder."""
    buf = (C.c_uint8 * 64)()
    n4 = (C.c_int32 * 4)()
    pcm = (C.c_float * 16)()
    b, nn, pc = C.addressof(buf), C.addressof(n4), C.addressof(pcm)
    crop = [P, I, P, LL, P, P, I, P, I, P, P, P, I, P, P]
    forms = []
    for name, tail in (("ulcx_decode_crops_dev", [P]), ("ulcx_decode_crops_dev_pcm16", [P]), ("ulcx_decode_crops_host", [])):
        fn = getattr(lib, name)
        fn.argtypes = crop + tail
        forms.append((name, fn, [None] * len(tail)))

    def call(fn, tail, nFiles=3, pay=b, nb=nn, idx=b, cnt=nn, n=2, file=nn, first=nn, count=None, nBlocks=2, out=pc, bits=nn):
        return fn(None, nFiles, pay, 64, nb, idx, 5, cnt, n, file, first, count, nBlocks, out, bits, *tail)

    for name, fn, tail in forms:
        def refused(why, **kw):
            assert call(fn, tail, **kw) == ERR_ARG, (name, kw)
            msg = lib.ulcx_last_error().decode()
            assert msg.startswith(name + ":") and why in msg, (name, kw, msg)
        for k in ("pay", "nb", "idx", "cnt", "file", "first", "out", "bits"):
            refused("NULL pointer", **{k: None}, n=0, nFiles=0, nBlocks=0)
        refused("(n 0)", n=0, nFiles=0, nBlocks=0)
        refused("(n -2)", n=-2)
        refused("(nFiles 0)", nFiles=0, nBlocks=0)
        refused("(nFiles -1)", nFiles=-1, nBlocks=99)
        refused("nBlocks is 1 .. maxBlocksPerCall - 1", nBlocks=0)
        refused("nBlocks is 1 .. maxBlocksPerCall - 1", nBlocks=-3)
        refused("no decoder")
        refused("no decoder", count=nn)
    lib.ulcx_index_packed_rows_dev.argtypes = [P, I, P, LL, P, I, P, P, P]
    lib.ulcx_index_packed_rows_host.argtypes = [P, I, P, LL, P, I, P, P]
    for rows, mb in ((5, 4), (0, 4), (5, 0), (-1, -3)):
        assert lib.ulcx_index_packed_rows_dev(None, rows, b, 64, nn, mb, b, nn, None) == ERR_ARG
        assert lib.ulcx_index_packed_rows_host(None, rows, b, 64, nn, mb, b, nn) == ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------
# corpus.py in front of freeze(): host logic
# ---------------------------------------------------------------------------------------------------------------------
def _ulc(bs, ch, n_blocks, payload, offs=24):
    return struct.pack("<IHHIIHHI", 0x32434C55, bs, 0, n_blocks, 44100, ch, 0, offs) + bytes(offs - 24) + payload      # tools/ulc_Helper.h:10-20


def _index(offs):
    import ulc_amd
    row = ulc_amd.new_index(1, len(offs))[0]
    row["ByteOffs"] = offs
    row["RngState"][1:] = np.arange(1, len(offs)) * 977
    return row


def test_corpus_parses_ulc_and_ulx(lib):
    import ulc_amd
    import corpus
    pay = bytes(range(200))
    h, p = corpus.parse_ulc(_ulc(2048, 2, 3, pay, offs=40))
    assert (h.BlockSize, h.nChan, h.nBlocks, h.StreamOffs) == (2048, 2, 3, 40) and p == pay
    for bad in (b"RIFF" + bytes(60), _ulc(2048, 2, 3, pay)[:20], struct.pack("<IHHIIHHI", 0x32434C55, 2048, 0, 3, 44100, 2, 0, 5000) + pay):
        with pytest.raises(ulc_amd.UlcError):
            corpus.parse_ulc(bad)
    cc = corpus.CropCorpus(2, 2048)
    row = _index([0, 50, 120, 200])
    assert cc.add_file(_ulc(2048, 2, 3, pay), ulc_amd.ulx_pack(row, 3, 2048, 2, len(pay))) == 0
    assert cc.add_file(_ulc(2048, 2, 7, pay[:90])) == 1
    assert len(cc) == 2
    lay = cc.layout()
    assert np.array_equal(lay["index"][0, :4], row) and lay["index_blocks"].tolist() == [3, 0] and lay["to_index"].tolist() == [1]


def test_corpus_refuses_another_geometry_and_a_stale_index(lib):
    import ulc_amd
    import corpus
    pay = bytes(range(200))
    row = _index([0, 50, 120, 200])
    cc = corpus.CropCorpus(2, 2048)
    with pytest.raises(ulc_amd.UlcError, match="BlockSize 1024"):
        cc.add_file(_ulc(1024, 2, 3, pay))
    with pytest.raises(ulc_amd.UlcError, match="1 channels"):
        cc.add_file(_ulc(2048, 1, 3, pay))
    with pytest.raises(ulc_amd.UlcError, match="index of BlockSize 4096"):
        cc.add_file(_ulc(2048, 2, 3, pay), ulc_amd.ulx_pack(row, 3, 4096, 2, len(pay)))
    with pytest.raises(ulc_amd.UlcError, match="payload of 199 bytes"):                  # stale: made for another payload size
        cc.add_file(_ulc(2048, 2, 3, pay), ulc_amd.ulx_pack(row, 3, 2048, 2, len(pay) - 1))
    with pytest.raises(ulc_amd.UlcError, match="ulcx_index_check"):                      # the right size, entries that run past it
        cc.add_file(_ulc(2048, 2, 3, pay), ulc_amd.ulx_pack(_index([0, 50, 120, 201]), 3, 2048, 2, len(pay)))
    with pytest.raises(ulc_amd.UlcError):                                                # a truncated sidecar
        cc.add_file(_ulc(2048, 2, 3, pay), ulc_amd.ulx_pack(row, 3, 2048, 2, len(pay))[:-3])
    assert len(cc) == 0
    with pytest.raises(ulc_amd.UlcError, match="no files"):
        cc.layout()


def test_corpus_layout_strides_and_offsets(lib):
    import ulc_amd
    import corpus
    rng = np.random.default_rng(5)
    sizes, blocks = [301, 5000, 77, 4999], [3, 40, 1, 12]
    pays = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in sizes]
    rows = {1: _index(np.linspace(0, sizes[1], 41).astype(np.int64)), 2: _index([0, 77])}
    cc = corpus.CropCorpus(1, 512)
    for f, (p, k) in enumerate(zip(pays, blocks)):
        cc.add_file(_ulc(512, 1, k, p), ulc_amd.ulx_pack(rows[f], k, 512, 1, len(p)) if f in rows else None)
    lay = cc.layout()
    stride = (5000 + 64 + 15) & ~15
    assert lay["stride"] == stride and lay["index_stride"] == 41
    assert lay["payload"].shape == (4, stride) and lay["payload"].dtype == np.uint8 and lay["payload"].flags["C_CONTIGUOUS"]
    flat = lay["payload"].reshape(-1)
    for f, p in enumerate(pays):                           # file f starts at byte f * stride, zeros behind it
        assert flat[f * stride:f * stride + len(p)].tobytes() == p and not flat[f * stride + len(p):(f + 1) * stride].any()
    assert lay["payload_bytes"].dtype == np.int32 and lay["payload_bytes"].tolist() == sizes
    assert lay["index"].shape == (4, 41) and lay["index"].dtype == ulc_amd.INDEX_DTYPE
    assert lay["index_blocks"].tolist() == [0, 40, 1, 0] and lay["to_index"].tolist() == [0, 3]
    assert np.array_equal(lay["index"][1], rows[1]) and np.array_equal(lay["index"][2, :2], rows[2])
    open_row = ulc_amd.new_index(1, 41)[0]
    assert np.array_equal(lay["index"][0], open_row) and np.array_equal(lay["index"][3], open_row) and np.array_equal(lay["index"][2, 2:], open_row[2:])
    for f in (1, 2):
        assert ulc_amd.index_check(lay["index"][f], lay["index_blocks"][f], lay["payload_bytes"][f])
