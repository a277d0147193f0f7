"""Clips and the strided -> ragged corpus call (include/ulc_amd.h section 3: ulcx_clip_blocks, ulcx_encode_clips_*,
ulcx_corpus_ragged_*) at the C-ABI boundary, without a GPU: exported symbols and their prototypes, the block arithmetic against
the tool's formula, every refusal that needs no device, and the numpy restatement of the ragged tables (clips_testlib.ragged_plan,
which the GPU tests hold the kernels to) against a hand-written table of cases, and the properties of clips_testlib's case tables
that tests/test_gpu_clips_paths.py leans on (block counts against chunk boundaries, window-switched blocks behind the first
chunk, rows whose rate search moves, capacities that cut where they say, every alignment pair of the byte copy)."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clips_testlib as ct

LIB = os.path.join(ROOT, "ulc-codec_amd", "libulc_amd.so")
NAMES = ("ulcx_clip_blocks", "ulcx_encode_clips_dev", "ulcx_encode_clips_dev_pcm16", "ulcx_encode_clips_host", "ulcx_corpus_ragged_dev", "ulcx_corpus_ragged_host")
ERR_ARG = -1
P, I, F, LL = C.c_void_p, C.c_int, C.c_float, C.c_longlong
CLIPS = [P, P, I, I, F, F, P, P, P, I, P, LL, P, P, P, I, P]
RAGGED = [I, I, P, LL, P, P, I, P, P, LL, P, P, LL, P, P, P]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ulc-codec_amd"), "-j8"], stdout=subprocess.DEVNULL)
    l = C.CDLL(LIB)
    l.ulcx_last_error.restype = C.c_char_p
    l.ulcx_clip_blocks.argtypes = [I, I]
    l.ulcx_encode_clips_dev.argtypes = CLIPS + [P]
    l.ulcx_encode_clips_dev_pcm16.argtypes = CLIPS + [P]
    l.ulcx_encode_clips_host.argtypes = CLIPS
    l.ulcx_corpus_ragged_dev.argtypes = RAGGED + [P]
    l.ulcx_corpus_ragged_host.argtypes = RAGGED
    return l


def test_entry_points_are_exported_and_bound(lib):
    import ulc_amd
    import corpus
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in ulc_amd.EXPORTS, n
    for m in ("encode_clips", "encode_clips_dev"):
        assert hasattr(ulc_amd.BatchEncoder, m), m
    for f in ("clip_blocks", "corpus_ragged_dev", "corpus_ragged"):
        assert hasattr(ulc_amd, f), f
    assert hasattr(corpus.CropCorpus, "from_clips")


def test_header_declares_the_entries_with_these_types():
    clips = ("ulcx_encoder *, ulcx_decoder *, int, int, float, float, const ulcx_rate *, const %s *, const int32_t *, int,\n"
             "         uint8_t *, long long, int32_t *, int32_t *, ulcx_index_entry *, int, int32_t *")
    ragged = ("int, int, const uint8_t *, long long, const int32_t *, const ulcx_index_entry *, int, const int32_t *,\n"
              "         uint8_t *, long long, int64_t *, ulcx_index_entry *, long long, int64_t *, int32_t *, int64_t *")
    src = ('#include "ulc_amd.h"\n'
           'int (*z)(int, int) = ulcx_clip_blocks;\n'
           f'int (*a)({clips % "float"}, void *) = ulcx_encode_clips_dev;\n'
           f'int (*b)({clips % "int16_t"}, void *) = ulcx_encode_clips_dev_pcm16;\n'
           f'int (*c)({clips % "float"}) = ulcx_encode_clips_host;\n'
           f'int (*d)({ragged}, void *) = ulcx_corpus_ragged_dev;\n'
           f'int (*e)({ragged}) = ulcx_corpus_ragged_host;\n'
           'int main(void){return 0;}\n')
    p = subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-"],
                       input=src.encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()


@pytest.mark.parametrize("bs", (256, 512, 2048, 32768))
def test_clip_blocks_is_the_tools_formula(lib, bs):
    import ulc_amd
    tool = lambda n: (n + bs - 1) // bs + 2                 # tools/ulcEncodeTool.c:93-98
    assert lib.ulcx_clip_blocks(bs, 0) == 0 and lib.ulcx_clip_blocks(bs, -5) == 0
    for n in (1, bs - 1, bs, bs + 1, 30 * bs + 1):
        assert lib.ulcx_clip_blocks(bs, n) == tool(n) == ulc_amd.clip_blocks(bs, n), n
    assert [lib.ulcx_clip_blocks(bs, n) for n in (1, bs - 1, bs, bs + 1)] == [3, 3, 3, 4]
    assert lib.ulcx_clip_blocks(bs, 0x7FFFFFFF) == tool(0x7FFFFFFF)
    for bad in (0, -bs, bs - 1, bs + 1, 128, 65536, 3 * bs):
        assert lib.ulcx_clip_blocks(bad, 5) == 0, bad


def _bufs():
    raw = (C.c_uint8 * 1024)()
    base = (C.addressof(raw) + 63) & ~63                    # 64-byte aligned, whatever ctypes gave
    return raw, base


def test_clip_refusals_without_a_device(lib):
    """Every ULCX_ERR_ARG of the clip calls that takes no device to see.  The objects are looked at last, so with NULL objects
    the message names the argument that was wrong - or "no encoder" when nothing else is."""
    _keep, p = _bufs()
    err = lambda: lib.ulcx_last_error().decode()
    good = dict(n=2, mode=0, rate=None, pcm=p, len=p + 64, nSamples=100, payload=p + 128, pstride=64, pbytes=p + 256, maxb=p + 320, index=p + 384, istride=4,
                iblocks=p + 448)

    def call(name, **kw):
        a = dict(good, **kw)
        args = [None, None, a["n"], a["mode"], 50.0, 0.0, a["rate"], a["pcm"], a["len"], a["nSamples"], a["payload"], a["pstride"], a["pbytes"], a["maxb"],
                a["index"], a["istride"], a["iblocks"]]
        return getattr(lib, name)(*(args + ([None] if "_dev" in name else [])))

    for name in ("ulcx_encode_clips_dev", "ulcx_encode_clips_dev_pcm16", "ulcx_encode_clips_host"):
        dev = "_dev" in name
        assert call(name) == ERR_ARG and err() == name + ": no encoder"
        assert call(name, len=None, maxb=None) == ERR_ARG and "no encoder" in err()          # the optional pointers
        for key in ("pcm", "payload", "pbytes", "index", "iblocks"):
            assert call(name, **{key: None}) == ERR_ARG and "NULL pointer" in err() and err().startswith(name + ":"), (name, key)
        for v in (0, -7):
            assert call(name, nSamples=v) == ERR_ARG and f"nSamples {v}" in err(), (name, v)
            assert call(name, pstride=v) == ERR_ARG and f"payloadStride {v}" in err(), (name, v)
            assert call(name, n=v) == ERR_ARG and f"(n {v})" in err(), (name, v)
        for v in (1, 0, -2):
            assert call(name, istride=v) == ERR_ARG and f"indexStride {v}" in err(), (name, v)
        for v in (3, -1):
            assert call(name, mode=v) == ERR_ARG and "bad mode" in err(), (name, v)
            assert call(name, mode=v, rate=p + 512) == ERR_ARG and "no encoder" in err(), (name, v)      # a table: the scalar mode is not looked at
        if not dev:
            continue
        # alignment: a sample of its own size (a plane starts anywhere), the table 8, the words 4, the payload none
        esz = 2 if "pcm16" in name else 4
        for off in range(1, esz):
            assert call(name, pcm=p + off) == ERR_ARG and f"not aligned to {esz} bytes" in err(), (name, off)
        assert call(name, pcm=p + esz) == ERR_ARG and "no encoder" in err()
        assert call(name, rate=p + 512 + 4) == ERR_ARG and "d_rate" in err() and "not aligned to 8 bytes" in err()
        for key in ("len", "pbytes", "maxb", "index", "iblocks"):
            for off in (1, 2, 3):
                assert call(name, **{key: good[key] + off}) == ERR_ARG and "not aligned to 4 bytes" in err(), (name, key, off)
        assert call(name, payload=p + 129) == ERR_ARG and "no encoder" in err()


def test_ragged_refusals_without_a_device(lib):
    _keep, p = _bufs()
    err = lambda: lib.ulcx_last_error().decode()
    good = dict(nFiles=2, payload=p, pstride=32, pbytes=p + 64, index=p + 128, istride=4, iblocks=p + 192, opay=p + 256, pcap=64, poffs=p + 320, oidx=p + 384,
                icap=8, ioffs=p + 448, oblocks=p + 512, need=p + 576)
    order = ("nFiles", "payload", "pstride", "pbytes", "index", "istride", "iblocks", "opay", "pcap", "poffs", "oidx", "icap", "ioffs", "oblocks", "need")

    def call(name, **kw):
        a = dict(good, **kw)
        return getattr(lib, name)(*([0] + [a[k] for k in order] + ([None] if "_dev" in name else [])))

    for name in ("ulcx_corpus_ragged_dev", "ulcx_corpus_ragged_host"):
        for key in ("payload", "pbytes", "index", "iblocks", "opay", "poffs", "oidx", "ioffs", "oblocks", "need"):
            assert call(name, **{key: None}) == ERR_ARG and "NULL pointer" in err() and err().startswith(name + ":"), (name, key)
        for key, word in (("nFiles", "nFiles"), ("pstride", "payloadStride"), ("istride", "indexStride")):
            for v in (0, -3):
                assert call(name, **{key: v}) == ERR_ARG and f"{word} {v}" in err(), (name, key, v)
        for key, word in (("pcap", "payloadCap"), ("icap", "indexCap")):
            assert call(name, **{key: -1}) == ERR_ARG and f"{word} -1" in err(), (name, key)
    name = "ulcx_corpus_ragged_dev"
    for key in ("poffs", "ioffs", "need"):
        assert call(name, **{key: good[key] + 4}) == ERR_ARG and "not aligned to 8 bytes" in err(), key
    for key in ("pbytes", "index", "iblocks", "oidx", "oblocks"):
        assert call(name, **{key: good[key] + 2}) == ERR_ARG and "not aligned to 4 bytes" in err(), key


# (bytes per file, blocks per file, payload stride, index stride, payload cap, index cap) -> (payload offs, index offs, blocks out, need)
RAGGED_CASES = [
    # everything fits: the exclusive prefix sums; a file's row is its blocks + 1 entries
    (([10, 0, 7], [2, 0, 1], 16, 4, 17, 7), ([0, 10, 10, 17], [0, 3, 4, 6], [2, 0, 1], [17, 6])),
    # the payload is one byte short of file 2: files 2 and 3 come out empty, the need is the whole corpus's
    (([10, 5, 7, 1], [2, 1, 1, 0], 16, 4, 21, 100), ([0, 10, 15, 15, 15], [0, 3, 5, 5, 5], [2, 1, 0, 0], [23, 8])),
    # a file behind the one that does not fit would fit by itself: it stays out all the same
    (([10, 9, 1], [1, 1, 1], 16, 4, 12, 100), ([0, 10, 10, 10], [0, 2, 2, 2], [1, 0, 0], [20, 6])),
    # the index is the capacity that runs out
    (([4, 4, 4], [3, 3, 3], 8, 4, 100, 7), ([0, 4, 4, 4], [0, 4, 4, 4], [3, 0, 0], [12, 12])),
    # clamped counts: bytes to [0, stride], blocks to [0, index_stride - 1]
    (([40, -3, 8], [9, -1, 2], 16, 4, 100, 100), ([0, 16, 16, 24], [0, 4, 5, 8], [3, 0, 2], [24, 8])),
    # zero files of payload: nothing laid out, every row is its closing entry
    (([0, 0], [0, 0], 16, 4, 0, 2), ([0, 0, 0], [0, 1, 2], [0, 0], [0, 2])),
    # no capacity at all: a sizing call
    (([10, 5], [2, 1], 16, 4, 0, 0), ([0, 0, 0], [0, 0, 0], [0, 0], [15, 5])),
]


@pytest.mark.parametrize("case", range(len(RAGGED_CASES)))
def test_ragged_plan_restates_the_rule(case):
    from clips_testlib import ragged_plan
    (nbytes, blocks, stride, istride, pcap, icap), want = RAGGED_CASES[case]
    got = ragged_plan(nbytes, stride, blocks, istride, pcap, icap)
    for g, w in zip(got, want):
        assert g.tolist() == w, (case, [x.tolist() for x in got])


# ---------------------------------------------------------------------------------------------------------------------
# What tests/test_gpu_clips_paths.py leans on, from clips_testlib and the oracle alone: a GPU test there cannot pass because
# its inputs miss the path it is named for.
# ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("geom", ct.PATH_GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_path_rows_end_at_every_position_of_a_chunk(geom):
    bs, ch, streams, maxk = geom
    case, rows = ct.path_case(bs), ct.path_rows(bs, ch)
    assert case.T == 20 * bs + 3 and ct.clip_blocks(bs, case.T) == 23
    assert [ct.clip_blocks(bs, n) for n in case.lengths] == ct.PATH_BLOCKS == [0, 3, 8, 9, 16, 17, 23]
    refs = ct.refs(bs, ch, case=case, rows=rows)
    assert [r.nb for r in refs] == [ct.PATH_BLOCKS[i] for i in rows] and len(rows) <= streams
    assert set(rows) >= {1, 3, 6}                           # inside the first chunk, one block into the second, the short last chunk
    chunks = [min(maxk, 23 - k0) for k0 in range(0, 23, maxk)]
    assert chunks == {8: [8, 8, 7], 6: [6, 6, 6, 5], 2: [2] * 11 + [1]}[maxk]
    wave = ct.wave(bs, ch, case.T)
    for i in rows:                                          # samples behind a row's length are not zero
        assert case.lengths[i] == case.T or np.abs(wave[i][:, case.lengths[i]:]).max() > 0.01, i
    if (bs, ch) == (16384, 1):
        return
    # decimated blocks go through k_pack, un-decimated ones through the direct packing: both behind the first chunk
    wc = np.concatenate([r.wc[maxk:] for r in refs])
    assert (wc != 0x10).any() and (wc == 0x10).any(), [hex(w) for w in wc]


@pytest.mark.parametrize("geom", ct.PATH_GEOMS[:2], ids=lambda g: f"{g[0]}x{g[1]}")
def test_path_table_rows_search_their_rate(geom):
    bs, ch = geom[:2]
    case = ct.path_case(bs)
    vbr, tab = ct.refs(bs, ch, case=case), ct.refs(bs, ch, table=True, case=case)
    searched = [i for i in range(7) if ct.TABLE[i][0] > 0 and tab[i].nb and not np.array_equal(tab[i].sizes, vbr[i].sizes)]
    assert searched, "no CBR or ABR row differs from VBR 50"
    assert any(not np.array_equal(tab[i].sizes[geom[3]:], vbr[i].sizes[geom[3]:]) for i in searched), "... behind the first chunk"


def test_path_capacities_cut_inside_the_second_chunk():
    bs, ch, _, maxk = ct.PATH_GEOMS[0]
    refs = ct.refs(bs, ch, case=ct.path_case(bs))
    pstride, istride = ct.path_cut_strides(refs)
    nb = 23
    whole = (refs[0].slot * nb, nb + 1)                     # the strides that hold every row in full
    assert refs[6].kept(pstride, whole[1]) == 10 and maxk + 1 <= 10 < 2 * maxk < refs[6].nb
    assert pstride == int(refs[6].sizes[:11].sum()) - 1
    assert len([r for r in refs if r.kept(pstride, whole[1]) == r.nb]) >= 2            # rows that fit, to be unchanged
    assert istride - 1 == 9 and [r.kept(whole[0], istride) for r in refs] == [0, 3, 8, 9, 9, 9, 9]


def test_grid_rows():
    bs, ch, streams, maxk = ct.GRID_GEOM
    case = ct.grid_case(bs)
    assert (bs, ch, maxk) == (256, 1, 2) and streams == 16384 + 5 and (streams - 1) // 16384 == 1
    assert case.T == 2 * bs + 1 and case.lengths == (0, 1, bs - 1, bs, bs + 1, 2 * bs, case.T)
    refs = ct.refs(bs, ch, case=case)
    assert [r.nb for r in refs] == [0, 3, 3, 3, 4, 4, 5]
    assert len({r.payload.tobytes() for r in refs}) == 7     # a row that got another row's clip is seen


def test_ragged_tile_corpora_cut_where_they_say():
    for F in ct.TILE_FILES:
        c = ct.corpus_tiles(F)
        assert c.pay.shape == (F, ct.TILE_STRIDE) and ct.TILE_STRIDE % 2 == 1 and c.index.shape == (F, 4)
        assert c.nbytes.min() >= 0 and c.nbytes.max() <= ct.TILE_STRIDE and (F < 200 or (c.nbytes.min() == 0 and c.nbytes.max() == ct.TILE_STRIDE))
        for what, pcap, icap, cut in ct.tile_caps(F):
            assert ct.cut_file(c, pcap, icap) == cut, (F, what)
    cuts = {what: cut for what, _, _, cut in ct.tile_caps(513)}
    assert sorted(cuts.values()) == [0, 256, 300, 400, 512, 513, 513]
    assert cuts["cut at exactly 256 files"] == 256 and 257 <= cuts["cut inside the second tile"] <= 511 and cuts["cut inside the third tile"] == 512
    assert cuts["the first file does not fit"] == 0
    # the index capacity is the one that cuts: the payload capacity alone would keep more files
    what, pcap, icap, cut = ct.tile_caps(513)[-1]
    assert cut == 300 < ct.cut_file(ct.corpus_tiles(513), pcap, ct.NO_CAP) == 450 and ct.cut_file(ct.corpus_tiles(513), ct.NO_CAP, icap) == 300
    assert [cut for _, _, _, cut in ct.tile_caps(1000)][-1] == 700 > 512


def test_ragged_untrusted_corpus_holds_the_values():
    c = ct.corpus_untrusted()
    S = ct.TILE_STRIDE
    assert c.pay.shape[0] == 300
    assert {-1, -2 ** 31, S + 1, 2 ** 31 - 1} <= set(c.nbytes.tolist()) and {-1, ct.RAGGED_ISTRIDE, 2 ** 31 - 1} <= set(c.blocks.tolist())
    poffs, ioffs, blocks, need = ct.plan_of(c)
    b, e = np.diff(poffs), np.diff(ioffs)
    assert b[3] == 0 and b[100] == 0 and b[200] == S and b[259] == S and e[5] == 1 and e[150] == 4 and e[270] == 4
    assert 0 <= b.min() and b.max() <= S and 1 <= e.min() and e.max() <= ct.RAGGED_ISTRIDE and need.tolist() == [b.sum(), e.sum()]


def test_ragged_byte_copy_corpus_covers_every_alignment_pair():
    c = ct.corpus_bytecopy()
    assert c.pay.shape == (64, ct.COPY_STRIDE) and {(f * ct.COPY_STRIDE) & 3 for f in range(64)} == {0, 1, 2, 3}
    assert set(c.nbytes.tolist()) == set(ct.COPY_SIZES) | {4 * 256 * 2 + 3, 4 * 256 + 1}
    poffs = ct.plan_of(c)[0]
    pairs = {(int(poffs[f]) & 3, (f * ct.COPY_STRIDE) & 3) for f in range(64) if c.nbytes[f] >= 4}     # relative to 4-aligned bases
    assert len(pairs) == 16
    for size in range(4):
        assert len({int(poffs[f]) & 3 for f in range(64) if c.nbytes[f] == size}) >= 2, size
    F = ct.corpus_many().pay.shape[0]
    assert F == 16384 + 3 and ct.corpus_many().nbytes.max() == 9 and ct.corpus_many().blocks.max() == 2
