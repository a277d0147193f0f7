"""The clips ladder calls (include/ulc_amd.h section 3: ulcx_encode_clips_ladder_*, ULCX_RUNG_AUTO) at the C-ABI boundary, without
a GPU: the exported symbols and their prototypes, every refusal that needs no device, and - from the oracle alone - the properties
of the inputs that tests/test_gpu_clips_ladder.py and tests/test_gpu_clips_ladder_paths.py lean on: a GPU test there cannot pass
because two rungs, two rows or AUTO and CBR happen to give the same bytes."""
import ctypes as C
import itertools
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import clips_testlib as ct
import clips_ladder_testlib as lt

LIB = os.path.join(ROOT, "ulc-codec_amd", "libulc_amd.so")
NAMES = ("ulcx_encode_clips_ladder_dev", "ulcx_encode_clips_ladder_dev_pcm16", "ulcx_encode_clips_ladder_host")
ERR_ARG = -1
P, I, F, LL = C.c_void_p, C.c_int, C.c_float, C.c_longlong


class Rung(C.Structure):
    _fields_ = [("mode", C.c_int32), ("param0", C.c_float), ("param1", C.c_float), ("reserved", C.c_int32), ("rate", C.c_void_p)]


LADDER = [P, P, I, C.POINTER(Rung), I, P, P, I, P, LL, P, P, P, I, P, P]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ulc-codec_amd"), "-j8"], stdout=subprocess.DEVNULL)
    l = C.CDLL(LIB)
    l.ulcx_last_error.restype = C.c_char_p
    for n in NAMES:
        getattr(l, n).argtypes = LADDER + ([P] if "_dev" in n else [])
    l.ulcx_encode_dev_ladder.argtypes = [P, C.POINTER(Rung), I, P, I, P, P, P, P, P]
    return l


def test_entry_points_are_exported_and_bound(lib):
    import ulc_amd
    import corpus
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in ulc_amd.EXPORTS, n
    for m in ("encode_clips_ladder", "encode_clips_ladder_dev"):
        assert hasattr(ulc_amd.BatchEncoder, m), m
    assert ulc_amd.RUNG_AUTO == 1
    assert hasattr(corpus.CropCorpus, "from_clips_ladder")


def test_header_declares_the_entries_with_these_types():
    args = ("ulcx_encoder *, ulcx_decoder *, int, const ulcx_rung *, int, const %s *, const int32_t *, int,\n"
            "         uint8_t *, long long, int32_t *, int32_t *, ulcx_index_entry *, int, int32_t *, float *")
    src = ('#include "ulc_amd.h"\n'
           f'int (*a)({args % "float"}, void *) = ulcx_encode_clips_ladder_dev;\n'
           f'int (*b)({args % "int16_t"}, void *) = ulcx_encode_clips_ladder_dev_pcm16;\n'
           f'int (*c)({args % "float"}) = ulcx_encode_clips_ladder_host;\n'
           '_Static_assert(ULCX_RUNG_AUTO == 1, "ULCX_RUNG_AUTO");\n'
           'int main(void){return 0;}\n')
    p = subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-"],
                       input=src.encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()


def _bufs():
    raw = (C.c_uint8 * 2048)()
    base = (C.addressof(raw) + 63) & ~63                    # 64-byte aligned, whatever ctypes gave
    return raw, base


def _rungs(*specs):
    """specs: (mode, p0, p1, reserved, rate address)"""
    arr = (Rung * max(len(specs), 1))()
    for r, s in enumerate(specs):
        arr[r].mode, arr[r].param0, arr[r].param1, arr[r].reserved, arr[r].rate = s
    return arr


def test_ladder_refusals_without_a_device(lib):
    """Every ULCX_ERR_ARG of the clips ladder calls that takes no device to see.  The objects are looked at last, so with NULL
    objects the message names the argument that was wrong - or "no encoder" when nothing else is."""
    _keep, p = _bufs()
    err = lambda: lib.ulcx_last_error().decode()
    table = p + 512
    two = _rungs((0, 50.0, 0.0, 0, None), (2, 64.0, 0.0, 1, None))
    good = dict(n=2, rungs=two, nRungs=2, pcm=p, len=p + 64, nSamples=100, payload=p + 128, pstride=64, pbytes=p + 256, maxb=p + 320, index=p + 384, istride=4,
                iblocks=p + 448, avg=p + 640)

    def call(name, **kw):
        a = dict(good, **kw)
        args = [None, None, a["n"], a["rungs"], a["nRungs"], a["pcm"], a["len"], a["nSamples"], a["payload"], a["pstride"], a["pbytes"], a["maxb"],
                a["index"], a["istride"], a["iblocks"], a["avg"]]
        return getattr(lib, name)(*(args + ([None] if "_dev" in name else [])))

    for name in NAMES:
        dev = "_dev" in name
        assert call(name) == ERR_ARG and err() == name + ": no encoder"
        assert call(name, len=None, maxb=None, avg=None) == ERR_ARG and "no encoder" in err()          # the optional pointers
        # what the clips call refuses
        for key in ("pcm", "payload", "pbytes", "index", "iblocks"):
            assert call(name, **{key: None}) == ERR_ARG and "NULL pointer" in err() and err().startswith(name + ":"), (name, key)
        for v in (0, -7):
            assert call(name, nSamples=v) == ERR_ARG and f"nSamples {v}" in err(), (name, v)
            assert call(name, pstride=v) == ERR_ARG and f"payloadStride {v}" in err(), (name, v)
            assert call(name, n=v) == ERR_ARG and f"(n {v})" in err(), (name, v)
        for v in (1, 0, -2):
            assert call(name, istride=v) == ERR_ARG and f"indexStride {v}" in err(), (name, v)
        # what ulcx_encode_dev_ladder refuses, except `reserved`
        assert call(name, rungs=None) == ERR_ARG and "nRungs" in err()
        for v in (0, -1, 9):
            assert call(name, nRungs=v) == ERR_ARG and f"nRungs {v} not in 1 .. 8" in err(), (name, v)
        for v in (3, -1):
            assert call(name, rungs=_rungs((0, 50.0, 0.0, 0, None), (v, 50.0, 0.0, 0, None))) == ERR_ARG and f"rung 1: bad mode {v}" in err(), (name, v)
            assert call(name, rungs=_rungs((0, 50.0, 0.0, 0, None), (v, 50.0, 0.0, 0, table))) == ERR_ARG and "no encoder" in err()     # a table: the mode is not looked at
        # `reserved`: 0 or ULCX_RUNG_AUTO
        for v in (2, 3, -1, 0x101):
            assert call(name, rungs=_rungs((0, 50.0, 0.0, 0, None), (1, 64.0, 0.0, v, None))) == ERR_ARG and "rung 1: reserved" in err() and "ULCX_RUNG_AUTO" in err(), (name, v)
        assert call(name, rungs=_rungs((1, 64.0, 0.0, 1, None), (0, 1.0, 9.0, 1, table))) == ERR_ARG and "no encoder" in err()        # AUTO on CBR and on a table
        # AUTO on a scalar rung needs a rate
        assert call(name, rungs=_rungs((2, 64.0, 0.0, 1, None), (0, 50.0, 0.0, 1, None))) == ERR_ARG and "rung 1: ULCX_RUNG_AUTO on a VBR rung" in err()
        for v in (0.0, -64.0, float("nan"), float("inf")):
            assert call(name, rungs=_rungs((2, v, 0.0, 1, None)), nRungs=1) == ERR_ARG and "rung 0: ULCX_RUNG_AUTO with RateKbps" in err(), (name, v)
        # nRungs * n files of indexStride entries beyond what ulcx_index_slots_dev takes in one call (0x7FFFFFFF << 8 entries), or
        # more files than an int counts: refused in front of the object checks, with the file count formed in 64 bits
        lim = 0x7FFFFFFF << 8
        eight = _rungs(*[(0, 50.0, 0.0, 0, None)] * 8)
        for nr, n, ist in ((8, 1 << 26, 2048), (1, 0x7FFFFFFF, 257), (8, 70, 1 << 30), (8, 70, lim // 560 + 1), (2, 0x7FFFFFFF, 2), (8, 1 << 29, 2)):
            assert nr * n * ist > lim or nr * n > 0x7FFFFFFF
            assert call(name, rungs=eight, nRungs=nr, n=n, istride=ist) == ERR_ARG, (name, nr, n, ist)
            assert err() == f"{name}: {nr * n} rows of {ist} entries are more than one call takes", (name, nr, n, ist, err())
        for nr, n, ist in ((1, 0x7FFFFFFF, 256), (8, 70, lim // 560), (4, 70, 1 << 30)):          # at and below the limit: the next check speaks
            assert nr * n * ist <= lim
            assert call(name, rungs=eight, nRungs=nr, n=n, istride=ist) == ERR_ARG and err() == name + ": no encoder", (name, nr, n, ist, err())
        if not dev:
            continue
        esz = 2 if "pcm16" in name else 4
        for off in range(1, esz):
            assert call(name, pcm=p + off) == ERR_ARG and f"not aligned to {esz} bytes" in err(), (name, off)
        assert call(name, pcm=p + esz) == ERR_ARG and "no encoder" in err()
        assert call(name, rungs=_rungs((0, 50.0, 0.0, 0, None), (0, 0.0, 0.0, 1, table + 4))) == ERR_ARG and "a rung's rate table" in err() and "not aligned to 8 bytes" in err()
        for key in ("len", "pbytes", "maxb", "index", "iblocks", "avg"):
            for off in (1, 2, 3):
                assert call(name, **{key: good[key] + off}) == ERR_ARG and "not aligned to 4 bytes" in err() and ("d_avg" in err()) == (key == "avg"), (name, key, off)
        assert call(name, payload=p + 129) == ERR_ARG and "no encoder" in err()


def test_the_plain_clips_calls_refuse_too_many_entries_the_same_way(lib):
    """The one body serves the plain entries: the same refusal, with one rung."""
    _keep, p = _bufs()
    plain = [P, P, I, I, F, F, P, P, P, I, P, LL, P, P, P, I, P]
    for name in ("ulcx_encode_clips_dev", "ulcx_encode_clips_dev_pcm16", "ulcx_encode_clips_host"):
        fn = getattr(lib, name)
        fn.argtypes = plain + ([P] if "_dev" in name else [])
        tail = [None] if "_dev" in name else []
        call = lambda n, ist: fn(None, None, n, 0, 50.0, 0.0, None, p, p + 64, 100, p + 128, 64, p + 256, p + 320, p + 384, ist, p + 448, *tail)
        assert call(0x7FFFFFFF, 257) == ERR_ARG and lib.ulcx_last_error().decode() == f"{name}: {0x7FFFFFFF} rows of 257 entries are more than one call takes"
        assert call(0x7FFFFFFF, 256) == ERR_ARG and lib.ulcx_last_error().decode() == name + ": no encoder"


def test_the_streaming_ladder_still_refuses_a_reserved_value(lib):
    _keep, p = _bufs()
    rc = lib.ulcx_encode_dev_ladder(None, _rungs((1, 64.0, 0.0, 1, None)), 1, p, 1, p + 64, p + 128, None, None, None)
    assert rc == ERR_ARG and "rung 0: reserved must be 0" in lib.ulcx_last_error().decode()


def test_python_rungs_spell_auto():
    import ulc_amd
    arr = ulc_amd.BatchEncoder._rungs([(0, 50.0), ("auto", 96.0), ("auto_table", 0x1000), 0x2000, (2, 64.0, 1.5)], int)
    assert [(g.mode, g.param0, g.param1, g.reserved, g.rate) for g in arr] == [(0, 50.0, 0.0, 0, None), (2, 96.0, 0.0, 1, None), (0, 0.0, 0.0, 1, 0x1000),
                                                                                 (0, 0.0, 0.0, 0, 0x2000), (2, 64.0, 1.5, 0, None)]
    with pytest.raises(ulc_amd.UlcError):
        ulc_amd.BatchEncoder._rungs([("abr", 96.0)], int)


def test_from_clips_ladder_refuses_a_rate_it_cannot_read():
    """A rate is (mode, p0[, p1]), ("auto", kbps), ("auto_table", table) or a table [n][2]; anything else raises before the
    encoder is touched (the objects here are stand-ins with the geometry only)."""
    import types
    import torch
    import corpus
    import ulc_amd
    obj = types.SimpleNamespace(C=2, BS=256, slot=2 * 2 * 256 + 16)
    wave = torch.zeros((3, 2, 100))
    for bad, why in ((("abr", 64.0), "rate 1"), (("auto", "64"), "rate 1"), (np.zeros((2, 2), np.float32), "rate 1: a table of shape"),
                     (((-50.0, 0.0), (64.0, 0.0)), "rate 1: a table of shape"), ((0, 50.0, 0.0, 0.0), "rate 1: a table of shape"),
                     (("auto_table", np.zeros((3, 3), np.float32)), "rate 1: a table of shape")):
        with pytest.raises(ulc_amd.UlcError, match=why):
            corpus.CropCorpus.from_clips_ladder(obj, obj, wave, rates=[(0, 50.0), bad])
    with pytest.raises(ulc_amd.UlcError, match="file_of"):
        corpus.CropCorpus(2, 256).file_of(0, 0)


def test_avg_is_the_sequential_binary64_sum():
    """avg_of against a hand case where the order and the width of the sum show: binary32 accumulation, or pairwise sums, give
    another value."""
    x = np.array([1e8, 1.0, -1e8, 0.25, 3.0], np.float32)
    assert lt.avg_of(x) == np.float32((((1e8 + 1.0) - 1e8 + 0.25) + 3.0) / 5) == np.float32(0.85)
    acc = np.float32(0)
    for v in x:
        acc = np.float32(acc + v)
    assert np.float32(acc / np.float32(5)) != lt.avg_of(x)
    assert lt.avg_of(np.zeros(0, np.float32)) == 0 and lt.avg_of(np.zeros(3, np.float32)) == 0


# ---------------------------------------------------------------------------------------------------------------------
# The premises of the GPU tests, from the oracle alone
# ---------------------------------------------------------------------------------------------------------------------
def _same_setting(bs, ch, i, a, b):
    return tuple(np.float32(lt.setting(bs, ch, i, a))) == tuple(np.float32(lt.setting(bs, ch, i, b)))


@pytest.mark.parametrize("geom", ct.GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_rungs_rows_and_auto_can_be_told_apart(geom):
    bs, ch = geom
    refs = lt.refs(bs, ch, lt.FIVE)
    assert [r.nb for r in refs[0]] == [0, 3, 3, 3, 4, 6, 8]
    # The rungs' payloads of a row differ pairwise wherever the rungs hand the row different settings.  The five rungs the GPU test
    # is given cannot differ on every row: TABLE's row 1 is CBR 64, the scalar rung 2; its row 2 is 96 kbps, so AUTO on TABLE gives
    # it what AUTO 96 gives it; the VBR rows of TABLE stay what they are under AUTO (rows 3 and 6), the rule under test there.  Row 1
    # is ONE sample: its three blocks are all but empty and two rates may write the same bytes, so it is not asked to tell rates
    # apart.  Rows 4 and 5 have five different settings and must give five different files.
    same = []
    for i in range(1, 7):
        for a, b in itertools.combinations(range(5), 2):
            if _same_setting(bs, ch, i, lt.FIVE[a], lt.FIVE[b]):
                same.append((i, a, b))
            elif i >= 2:
                assert refs[a][i].payload.tobytes() != refs[b][i].payload.tobytes(), f"row {i}: rungs {a} and {b} write the same bytes"
    assert same == [(1, 1, 2), (2, 3, 4), (3, 1, 4), (6, 1, 4)]
    for i in (4, 5):
        assert len({refs[r][i].payload.tobytes() for r in range(5)}) == 5, i
    # the averages: pairwise different and > 0
    avgs = [lt.avg(bs, ch, i) for i in range(7)]
    assert avgs[0] == 0 and all(a > 0 for a in avgs[1:]) and len(set(float(a) for a in avgs[1:])) == 6, avgs
    # AUTO is neither CBR nor another row's average, for at least one row
    told = []
    for i in range(1, 7):
        j = i % 6 + 1
        auto = refs[3][i].payload.tobytes()
        cbr = lt._ref(bs, ch, i, None, (96.0, 0.0)).payload.tobytes()
        swapped = lt._ref(bs, ch, i, None, tuple(float(x) for x in lt.setting(bs, ch, i, lt.AUTO96, avg_row=j))).payload.tobytes()
        if auto != cbr and auto != swapped:
            told.append(i)
    assert told, "no row tells AUTO 96 from CBR 96 and from a swapped average"


@pytest.mark.parametrize("geom", ct.GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_capacity_case_cuts_rungs_apart(geom):
    bs, ch = geom
    refs = lt.refs(bs, ch, lt.FIVE)
    hi, lo, m, stride = lt.ladder_cut(bs, ch)
    whole = ct.clip_blocks(bs, ct.n_samples(bs)) + 1
    assert hi != lo and refs[hi][6].kept(stride, whole) == m and 2 <= m < 8 == refs[lo][6].kept(stride, whole)      # cut in a chunk behind the first; the low rung whole
    assert len({refs[r][6].kept(stride, whole) for r in range(5)}) >= 2
    # indexStride - 1 = 4: below the longest row's 8 blocks under every rung
    assert [[refs[r][i].kept(1 << 30, 5) for i in range(7)] for r in range(5)] == [[0, 3, 3, 3, 4, 4, 4]] * 5


def test_path_case_premises():
    bs, ch, streams, maxk = ct.PATH_GEOMS[0]
    case = ct.path_case(bs)
    refs = lt.refs(bs, ch, lt.PATH_RUNGS, case)
    assert [r.nb for r in refs[1]] == ct.PATH_BLOCKS and (streams, maxk) == (70, 8)
    avgs = [lt.avg(bs, ch, i, case) for i in range(7)]
    assert avgs[0] == 0 and all(a > 0 for a in avgs[1:]) and len(set(float(a) for a in avgs[1:])) == 6, avgs
    for i in range(1, 7):
        assert len({refs[r][i].payload.tobytes() for r in range(3)}) == 3, i
    # AUTO 64 moves the rate search away from CBR 64 behind the first chunk, for some row
    assert any(not np.array_equal(refs[1][i].sizes[maxk:], lt._ref(bs, ch, i, case, (64.0, 0.0)).sizes[maxk:]) for i in range(2, 7))
    hi = int(np.argmax([refs[r][6].payload.size for r in range(3)]))
    pstride, istride = ct.path_cut_strides(refs[hi])
    assert refs[hi][6].kept(pstride, 24) == 10 and istride == 10
    assert len({refs[r][6].kept(pstride, 24) for r in range(3)}) >= 2          # the rungs of row 6 stop at different blocks


def test_grid_case_premises():
    bs, ch, streams, maxk = ct.GRID_GEOM
    refs = lt.refs(bs, ch, lt.GRID_RUNGS, ct.grid_case(bs))
    assert 2 * streams > 2 * 16384 and [r.nb for r in refs[1]] == [0, 3, 3, 3, 4, 4, 5]
    assert len({r.payload.tobytes() for g in refs for r in g[1:]}) >= 11       # (row 0 is empty; TABLE's row 0 setting is VBR 50 too)
