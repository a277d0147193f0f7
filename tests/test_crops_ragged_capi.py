"""Crops of a ragged corpus (include/ulc_amd.h section 3: ulcx_decode_crops_ragged_* / ulcx_index_packed_ragged_*) at the C-ABI
boundary and the ragged layout of ulc-codec_amd/corpus.py, without a GPU: exported symbols and their binding, the header as
C, the refusals that need no device in their order, and CropCorpus(layout="ragged").layout() on numpy arrays."""
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
NAMES = ("ulcx_decode_crops_ragged_dev", "ulcx_decode_crops_ragged_dev_pcm16", "ulcx_decode_crops_ragged_host",
         "ulcx_index_packed_ragged_dev", "ulcx_index_packed_ragged_host")
ERR_ARG = -1
P, I, LL = C.c_void_p, C.c_int, C.c_longlong


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ulc-codec_amd"), "-j8"], stdout=subprocess.DEVNULL)
    l = C.CDLL(LIB)
    l.ulcx_last_error.restype = C.c_char_p
    return l


def test_ragged_entry_points_are_exported_and_bound(lib):
    import ulc_amd
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in ulc_amd.EXPORTS, n
    for m in ("decode_crops_ragged", "decode_crops_ragged_dev", "index_packed_ragged", "index_packed_ragged_dev"):
        assert hasattr(ulc_amd.BatchDecoder, m), m


def test_header_compiles_as_c_and_declares_the_ragged_calls():
    crop = ('ulcx_decoder *, int, const uint8_t *, long long, const int64_t *, const ulcx_index_entry *, long long, const int64_t *,\n'
            '         const int32_t *, int, const int32_t *, const int32_t *, const int32_t *, int, ')
    idx = 'ulcx_decoder *, int, const uint8_t *, long long, const int64_t *, ulcx_index_entry *, long long, const int64_t *, int32_t *'
    src = ('#include "ulc_amd.h"\n'
           f'int (*a)({crop}float *, int32_t *, void *) = ulcx_decode_crops_ragged_dev;\n'
           f'int (*b)({crop}int16_t *, int32_t *, void *) = ulcx_decode_crops_ragged_dev_pcm16;\n'
           f'int (*c)({crop}float *, int32_t *) = ulcx_decode_crops_ragged_host;\n'
           f'int (*d)({idx}, void *) = ulcx_index_packed_ragged_dev;\n'
           f'int (*e)({idx}) = ulcx_index_packed_ragged_host;\n'
           'int main(void){return 0;}\n')
    p = subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-"],
                       input=src.encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()


def test_ragged_refusals_without_a_device_come_in_order(lib):
    """No object, so every call is refused before anything touches a device; which argument the refusal names shows the order of
    the checks: NULL pointers, n, nFiles, nBlocks, negative totals - and only then the missing decoder."""
    buf = (C.c_uint8 * 64)()
    n4 = (C.c_int32 * 4)()
    o4 = (C.c_int64 * 4)()
    pcm = (C.c_float * 16)()
    b, nn, oo, pc = C.addressof(buf), C.addressof(n4), C.addressof(o4), C.addressof(pcm)
    crop = [P, I, P, LL, P, P, LL, P, P, I, P, P, P, I, P, P]
    forms = []
    for name, tail in (("ulcx_decode_crops_ragged_dev", [P]), ("ulcx_decode_crops_ragged_dev_pcm16", [P]), ("ulcx_decode_crops_ragged_host", [])):
        fn = getattr(lib, name)
        fn.argtypes = crop + tail
        forms.append((name, fn, [None] * len(tail)))

    def call(fn, tail, nFiles=3, pay=b, ptot=64, poffs=oo, idx=b, itot=8, ioffs=oo, cnt=nn, n=2, file=nn, first=nn, count=None, nBlocks=2,
             out=pc, bits=nn):
        return fn(None, nFiles, pay, ptot, poffs, idx, itot, ioffs, cnt, n, file, first, count, nBlocks, out, bits, *tail)

    for name, fn, tail in forms:
        def refused(why, **kw):
            assert call(fn, tail, **kw) == ERR_ARG, (name, kw)
            msg = lib.ulcx_last_error().decode()
            assert msg.startswith(name + ":") and why in msg, (name, kw, msg)
        for k in ("pay", "poffs", "idx", "ioffs", "cnt", "file", "first", "out", "bits"):
            refused("NULL pointer", **{k: None}, n=0, nFiles=0, nBlocks=0, ptot=-1)
        refused("(n 0)", n=0, nFiles=0, nBlocks=0, itot=-1)
        refused("(n -2)", n=-2)
        refused("(nFiles 0)", nFiles=0, nBlocks=0, ptot=-1)
        refused("(nFiles -1)", nFiles=-1, nBlocks=99)
        refused("nBlocks is 1 .. maxBlocksPerCall - 1", nBlocks=0, ptot=-1)
        refused("nBlocks is 1 .. maxBlocksPerCall - 1", nBlocks=-3, itot=-1)
        refused("payloadTotal -1", ptot=-1)
        refused("indexTotal -5", itot=-5)
        refused("no decoder")
        refused("no decoder", count=nn, ptot=0, itot=0)
    lib.ulcx_index_packed_ragged_dev.argtypes = [P, I, P, LL, P, P, LL, P, P, P]
    lib.ulcx_index_packed_ragged_host.argtypes = [P, I, P, LL, P, P, LL, P, P]
    for files, ptot, itot in ((3, 64, 8), (0, 64, 8), (3, -1, 8), (3, 64, -1), (-1, -1, -1)):
        assert lib.ulcx_index_packed_ragged_dev(None, files, b, ptot, oo, b, itot, oo, nn, None) == ERR_ARG
        assert lib.ulcx_index_packed_ragged_host(None, files, b, ptot, oo, b, itot, oo, nn) == ERR_ARG
    for k in range(5):                                     # each pointer of the index call NULL in turn
        a = [b, oo, b, oo, nn]
        a[k] = None
        assert lib.ulcx_index_packed_ragged_dev(None, 3, a[0], 64, a[1], a[2], 8, a[3], a[4], None) == ERR_ARG
        assert lib.ulcx_index_packed_ragged_host(None, 3, a[0], 64, a[1], a[2], 8, a[3], a[4]) == ERR_ARG


# ---------------------------------------------------------------------------------------------------------------------
# corpus.py in front of freeze(): the ragged layout
# ---------------------------------------------------------------------------------------------------------------------
def _ulc(bs, ch, n_blocks, payload, offs=24):
    return struct.pack("<IHHIIHHI", 0x32434C55, bs, 0, n_blocks, 44100, ch, 0, offs) + bytes(offs - 24) + payload      # tools/ulc_Helper.h:10-20


def _index(offs):
    import ulc_amd
    row = ulc_amd.new_index(1, len(offs))[0]
    row["ByteOffs"] = offs
    row["RngState"][1:] = np.arange(1, len(offs)) * 977
    return row


SIZES, BLOCKS = [301, 5000, 77, 4999], [3, 40, 1, 12]


def _filled(layout=None):
    import ulc_amd
    import corpus
    rng = np.random.default_rng(5)
    pays = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in SIZES]
    rows = {1: _index(np.linspace(0, SIZES[1], 41).astype(np.int64)), 2: _index([0, 77])}
    cc = corpus.CropCorpus(1, 512) if layout is None else corpus.CropCorpus(1, 512, layout=layout)
    for f, (p, k) in enumerate(zip(pays, BLOCKS)):
        cc.add_file(_ulc(512, 1, k, p), ulc_amd.ulx_pack(rows[f], k, 512, 1, len(p)) if f in rows else None)
    return cc, pays, rows


def test_ragged_layout_offsets_rows_and_to_index(lib):
    import ulc_amd
    import corpus
    cc, pays, rows = _filled("ragged")
    lay = cc.layout()
    assert sorted(lay) == ["index", "index_blocks", "index_offs", "payload", "payload_offs", "to_index"]
    po, io = lay["payload_offs"], lay["index_offs"]
    assert po.dtype == np.int64 and io.dtype == np.int64 and po.shape == (5,) and io.shape == (5,)
    assert po.tolist() == [0] + np.cumsum(SIZES).tolist(), "payload offsets are not tight"
    assert (np.diff(po) >= 0).all() and (np.diff(io) >= 0).all()
    assert lay["payload"].dtype == np.uint8 and lay["payload"].ndim == 1 and lay["payload"].flags["C_CONTIGUOUS"]
    assert int(po[-1]) + corpus.PAYLOAD_PAD == lay["payload"].size
    assert not lay["payload"][po[-1]:].any()
    for f, p in enumerate(pays):
        assert lay["payload"][po[f]:po[f + 1]].tobytes() == p, f
    assert io.tolist() == [0] + np.cumsum([k + 1 for k in BLOCKS]).tolist(), "row f has blocks_f + 1 entries"
    assert lay["index"].dtype == ulc_amd.INDEX_DTYPE and lay["index"].shape == (int(io[-1]),)
    assert lay["index_blocks"].dtype == np.int32 and lay["index_blocks"].tolist() == [0, 40, 1, 0]
    assert lay["to_index"].tolist() == [0, 3]
    for f in (1, 2):                                       # a `.ulx` row is copied verbatim
        assert np.array_equal(lay["index"][io[f]:io[f + 1]], rows[f]), f
        assert ulc_amd.index_check(lay["index"][io[f]:io[f + 1]], lay["index_blocks"][f], SIZES[f])
    for f in (0, 3):                                       # a file to index: an open row of the header's block count + 1
        assert np.array_equal(lay["index"][io[f]:io[f + 1]], ulc_amd.new_index(1, BLOCKS[f] + 1)[0]), f
    with pytest.raises(ulc_amd.UlcError, match="layout"):
        corpus.CropCorpus(1, 512, layout="csr")
    with pytest.raises(ulc_amd.UlcError, match="no files"):
        corpus.CropCorpus(1, 512, layout="ragged").layout()


def test_strided_layout_is_the_default_and_unchanged(lib):
    import ulc_amd
    for cc, pays, rows in (_filled(), _filled("strided")):
        assert cc.ragged is False
        lay = cc.layout()
        assert sorted(lay) == ["index", "index_blocks", "index_stride", "payload", "payload_bytes", "stride", "to_index"]
        stride = (5000 + 64 + 15) & ~15
        assert lay["stride"] == stride and lay["index_stride"] == 41
        assert lay["payload"].shape == (4, stride) and lay["payload"].dtype == np.uint8
        for f, p in enumerate(pays):
            assert lay["payload"][f, :len(p)].tobytes() == p and not lay["payload"][f, len(p):].any()
        assert lay["payload_bytes"].dtype == np.int32 and lay["payload_bytes"].tolist() == SIZES
        assert lay["index"].shape == (4, 41) and lay["index"].dtype == ulc_amd.INDEX_DTYPE
        assert lay["index_blocks"].tolist() == [0, 40, 1, 0] and lay["to_index"].tolist() == [0, 3]
        open_row = ulc_amd.new_index(1, 41)[0]
        assert np.array_equal(lay["index"][1], rows[1]) and np.array_equal(lay["index"][2, :2], rows[2]) and np.array_equal(lay["index"][2, 2:], open_row[2:])
        assert np.array_equal(lay["index"][0], open_row) and np.array_equal(lay["index"][3], open_row)
