"""Clip spectra (include/ulc_amd.h section 3: ulcx_analyse_clips_*, ulcx_encode_clips_spectra_*) at the C-ABI boundary, without
a GPU: the six symbols exported, bound and declared with their types, every refusal that needs no device, and the properties of
the references (clip_spectra_testlib, from the oracle alone) that tests/test_gpu_clip_spectra.py and
tests/test_gpu_clip_spectra_paths.py lean on: decimated and un-decimated blocks in every geometry, behind the first chunk where
the call has several, and a shallow plane depth that cuts rows inside a chunk."""
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
import clip_spectra_testlib as cs
from spectra_testlib import to_lr

LIB = os.path.join(ROOT, "ulc-codec_amd", "libulc_amd.so")
ANALYSE = ("ulcx_analyse_clips_dev", "ulcx_analyse_clips_dev_pcm16", "ulcx_analyse_clips_host")
ENCODE = ("ulcx_encode_clips_spectra_dev", "ulcx_encode_clips_spectra_dev_pcm16", "ulcx_encode_clips_spectra_host")
ERR_ARG = -1
P, I, F, LL = C.c_void_p, C.c_int, C.c_float, C.c_longlong
ROWS = [P, I, P, P, I]                                      # enc, n, pcm, len, nSamples
CLIPS = [P, P, I, I, F, F, P, P, P, I, P, LL, P, P, P, I, P]
TAP = [I, I, P, P, P]                                       # nBlocks, flags, coef, wc, cplx


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ulc-codec_amd"), "-j8"], stdout=subprocess.DEVNULL)
    l = C.CDLL(LIB)
    l.ulcx_last_error.restype = C.c_char_p
    for name in ANALYSE + ENCODE:
        assert hasattr(l, name), f"{name} is not exported"
        getattr(l, name).argtypes = (ROWS if name in ANALYSE else CLIPS) + TAP + ([P] if "_dev" in name else [])
    return l


def test_entry_points_are_exported_and_bound(lib):
    import ulc_amd
    import corpus
    for n in ANALYSE + ENCODE:
        assert hasattr(lib, n), n
        assert n in ulc_amd.EXPORTS, n
    for m in ("analyse_clips", "analyse_clips_dev", "encode_clips_spectra", "encode_clips_spectra_dev"):
        assert hasattr(ulc_amd.BatchEncoder, m), m
    assert hasattr(corpus, "clip_spectra") and hasattr(corpus.CropCorpus, "from_clips_spectra")
    assert ulc_amd.SPECTRA_LR == cs.SPECTRA_LR == 1


def test_header_declares_the_entries_with_these_types():
    rows = "ulcx_encoder *, int, const %s *, const int32_t *, int"
    clips = ("ulcx_encoder *, ulcx_decoder *, int, int, float, float, const ulcx_rate *, const %s *, const int32_t *, int,\n"
             "         uint8_t *, long long, int32_t *, int32_t *, ulcx_index_entry *, int, int32_t *")
    tap = "int, int, float *, int32_t *, float *"
    src = ('#include "ulc_amd.h"\n'
           f'int (*a)({rows % "float"}, {tap}, void *) = ulcx_analyse_clips_dev;\n'
           f'int (*b)({rows % "int16_t"}, {tap}, void *) = ulcx_analyse_clips_dev_pcm16;\n'
           f'int (*c)({rows % "float"}, {tap}) = ulcx_analyse_clips_host;\n'
           f'int (*d)({clips % "float"}, {tap}, void *) = ulcx_encode_clips_spectra_dev;\n'
           f'int (*e)({clips % "int16_t"}, {tap}, void *) = ulcx_encode_clips_spectra_dev_pcm16;\n'
           f'int (*f)({clips % "float"}, {tap}) = ulcx_encode_clips_spectra_host;\n'
           'int flag = ULCX_SPECTRA_LR;\n'
           'int main(void){return 0;}\n')
    p = subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-"],
                       input=src.encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()


def _bufs():
    raw = (C.c_uint8 * 2048)()
    base = (C.addressof(raw) + 63) & ~63                    # 64-byte aligned, whatever ctypes gave
    return raw, base


def test_refusals_without_a_device(lib):
    """Every ULCX_ERR_ARG of the six entries that takes no device to see.  The objects are looked at last, so with NULL objects
    the message names the argument that was wrong - or "no encoder" when nothing else is."""
    _keep, p = _bufs()
    err = lambda: lib.ulcx_last_error().decode()
    good = dict(n=2, mode=0, rate=None, pcm=p, len=p + 64, nSamples=100, payload=p + 128, pstride=64, pbytes=p + 256, maxb=p + 320, index=p + 384, istride=4,
                iblocks=p + 448, nBlocks=3, flags=0, coef=p + 1024, wc=p + 640, cplx=p + 704)

    def call(name, **kw):
        a = dict(good, **kw)
        tap = [a["nBlocks"], a["flags"], a["coef"], a["wc"], a["cplx"]]
        if name in ANALYSE:
            args = [None, a["n"], a["pcm"], a["len"], a["nSamples"]] + tap
        else:
            args = [None, None, a["n"], a["mode"], 50.0, 0.0, a["rate"], a["pcm"], a["len"], a["nSamples"], a["payload"], a["pstride"], a["pbytes"], a["maxb"],
                    a["index"], a["istride"], a["iblocks"]] + tap
        return getattr(lib, name)(*(args + ([None] if "_dev" in name else [])))

    for name in ANALYSE + ENCODE:
        dev, encode = "_dev" in name, name in ENCODE
        assert call(name) == ERR_ARG and err() == name + ": no encoder"
        assert call(name, len=None, wc=None, cplx=None, flags=1) == ERR_ARG and "no encoder" in err()          # the optional pointers, ULCX_SPECTRA_LR
        # the tap's own refusals
        assert call(name, coef=None) == ERR_ARG and "no coefficient planes" in err() and err().startswith(name + ":"), name
        for v in (0, -3):
            assert call(name, nBlocks=v) == ERR_ARG and f"nBlocks {v}" in err(), (name, v)
        for v in (2, 3, 4, -1, 0x100):
            assert call(name, flags=v) == ERR_ARG and "bad flags" in err(), (name, v)
        # the clips call's refusals (an analysis form has no rate, corpus or decoder to refuse)
        assert call(name, pcm=None) == ERR_ARG and "NULL pointer" in err() and err().startswith(name + ":"), name
        for v in (0, -7):
            assert call(name, nSamples=v) == ERR_ARG and f"nSamples {v}" in err(), (name, v)
            assert call(name, n=v) == ERR_ARG and f"(n {v})" in err(), (name, v)
        if encode:
            for key in ("payload", "pbytes", "index", "iblocks"):
                assert call(name, **{key: None}) == ERR_ARG and "NULL pointer" in err(), (name, key)
            for v in (0, -7):
                assert call(name, pstride=v) == ERR_ARG and f"payloadStride {v}" in err(), (name, v)
            for v in (1, 0, -2):
                assert call(name, istride=v) == ERR_ARG and f"indexStride {v}" in err(), (name, v)
            for v in (3, -1):
                assert call(name, mode=v) == ERR_ARG and "bad mode" in err(), (name, v)
                assert call(name, mode=v, rate=p + 512) == ERR_ARG and "no encoder" in err(), (name, v)
        if not dev:
            continue
        # alignment: the planes 16 bytes, the words 4, a sample its own size, the table 8
        for off in (1, 2, 4, 8, 12):
            assert call(name, coef=good["coef"] + off) == ERR_ARG and "d_coef" in err() and "not aligned to 16 bytes" in err(), (name, off)
        assert call(name, coef=good["coef"] + 16) == ERR_ARG and "no encoder" in err()
        for key, what in (("wc", "d_wc"), ("cplx", "d_cplx"), ("len", "d_len")):
            for off in (1, 2, 3):
                assert call(name, **{key: good[key] + off}) == ERR_ARG and what in err() and "not aligned to 4 bytes" in err(), (name, key, off)
        esz = 2 if "pcm16" in name else 4
        for off in range(1, esz):
            assert call(name, pcm=p + off) == ERR_ARG and f"not aligned to {esz} bytes" in err(), (name, off)
        if encode:
            assert call(name, rate=p + 512 + 4) == ERR_ARG and "d_rate" in err() and "not aligned to 8 bytes" in err()
            for key in ("pbytes", "maxb", "index", "iblocks"):
                assert call(name, **{key: good[key] + 2}) == ERR_ARG and "not aligned to 4 bytes" in err(), (name, key)


# ---------------------------------------------------------------------------------------------------------------------
# What the GPU tests lean on, from clips_testlib's waves and the oracle alone
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ct.GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_short_references_hold_decimated_and_full_blocks(geom):
    bs, ch = geom
    refs = cs.specs(bs, ch)
    assert [r.nb for r in refs] == [0, 3, 3, 3, 4, 6, 8] == [ct.clip_blocks(bs, n) for n in ct.lengths(bs)]
    codes = {int(w) for r in refs for w in r.wc}
    assert codes == {0x10, 0x89 if geom == (512, 1) else 0x49}, [hex(w) for w in sorted(codes)]
    for r, c in zip(refs, ct.refs(bs, ch)):                 # the run is ClipRef's: the same window codes
        assert np.array_equal(r.wc, c.wc)
    live = np.concatenate([r.coef.reshape(-1) for r in refs])
    assert np.isfinite(live).all() and (live != 0).mean() > 0.5
    assert all((r.cplx > 0).any() for r in refs if r.nb)
    if ch > 1:                                              # LR is seen: the side channel is not silent
        assert not np.array_equal(to_lr(cs.expected(refs, 8)[0]), cs.expected(refs, 8)[0])


def test_shallow_depth_cuts_rows_inside_a_chunk():
    maxk = 2                                                # maxBlocksPerCall of tests/test_gpu_clip_spectra.py
    exact, shallow, deep = cs.DEPTHS
    nb = [ct.clip_blocks(256, n) for n in ct.lengths(256)]
    assert exact == max(nb) == ct.clip_blocks(256, ct.n_samples(256)) and exact % maxk == 0
    assert shallow % maxk == 1 and [i for i in range(7) if nb[i] > shallow] == [5, 6]      # the chunk of blocks 4 and 5: block 5 of rows 5 and 6 has no plane
    assert deep - exact == 3
    coef, wc, cplx = cs.expected(cs.specs(256, 2), shallow)
    assert coef.shape == (7, 2, shallow, 256) and (wc[5:] != 0).all() and (wc[4, 4:] == 0).all()
    coef, wc, cplx = cs.expected(cs.specs(256, 2), deep)
    assert not coef[:, :, exact:].any() and not wc[:, exact:].any() and not cplx[:, exact:].any() and coef[6, :, exact - 1].any()


@pytest.mark.parametrize("geom", ct.PATH_GEOMS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_path_references_hold_both_kinds_behind_the_first_chunk(geom):
    bs, ch, streams, maxk = geom
    case, rows = ct.path_case(bs), ct.path_rows(bs, ch)
    refs = cs.specs(bs, ch, case=case, rows=rows)
    assert [r.nb for r in refs] == [ct.PATH_BLOCKS[i] for i in rows]
    wc = np.concatenate([r.wc[maxk:] for r in refs])
    assert ((wc & 8) != 0).any() and (wc == 0x10).any(), [hex(w) for w in wc]


def test_grid_references():
    bs, ch, streams, maxk = ct.GRID_GEOM
    refs = cs.specs(bs, ch, case=ct.grid_case(bs))
    assert [r.nb for r in refs] == [0, 3, 3, 3, 4, 4, 5] and streams > 16384
    assert len({r.coef.tobytes() for r in refs}) == 7       # a row that got another row's clip is seen
