"""Spectra (include/ulc_amd.h section 3: ulcx_decode_crops_spectra_* / ulcx_window_subblocks) at the C-ABI boundary, without a
GPU: the sub-block arithmetic against the format's table and the oracle's, the four entries' presence and the refusals that need
no device, and the premises of tests/test_gpu_spectra.py's inputs - asserted here, counted with the decoder written from
FormatSpecs.md alone, together with the fact that the rows those tests name cover the blocks the properties live in."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
import spectra_testlib as S
from spec_decoder import _WINDOWS
from seek_testlib import ORACLE_CASES, oracle_stream

LIB = os.path.join(ROOT, "ulc-codec_amd", "libulc_amd.so")
NAMES = ("ulcx_window_subblocks", "ulcx_decode_crops_spectra_dev", "ulcx_decode_crops_spectra_host", "ulcx_decode_crops_spectra_ragged_dev",
         "ulcx_decode_crops_spectra_ragged_host")
ERR_ARG = -1
P, I, LL = C.c_void_p, C.c_int, C.c_longlong


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ulc-codec_amd"), "-j8"], stdout=subprocess.DEVNULL)
    l = C.CDLL(LIB)
    l.ulcx_last_error.restype = C.c_char_p
    return l


def test_spectra_entry_points_are_exported_and_bound(lib):
    import ulc_amd
    import corpus
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in ulc_amd.EXPORTS, n
    for m in ("decode_crops_spectra", "decode_crops_spectra_dev", "decode_crops_spectra_ragged", "decode_crops_spectra_ragged_dev"):
        assert hasattr(ulc_amd.BatchDecoder, m), m
    assert ulc_amd.SPECTRA_LR == 1 and callable(ulc_amd.window_subblocks) and hasattr(corpus.CropCorpus, "spectra")


def test_header_compiles_as_c_and_declares_the_calls():
    rows = 'int, const int32_t *, const int32_t *, const int32_t *, int, int, float *, int32_t *, int32_t *'
    strided = 'ulcx_decoder *, int, const uint8_t *, long long, const int32_t *, const ulcx_index_entry *, int, const int32_t *, '
    ragged = 'ulcx_decoder *, int, const uint8_t *, long long, const int64_t *, const ulcx_index_entry *, long long, const int64_t *, const int32_t *, '
    src = ('#include "ulc_amd.h"\n'
           f'int (*a)({strided}{rows}, void *) = ulcx_decode_crops_spectra_dev;\n'
           f'int (*b)({strided}{rows}) = ulcx_decode_crops_spectra_host;\n'
           f'int (*c)({ragged}{rows}, void *) = ulcx_decode_crops_spectra_ragged_dev;\n'
           f'int (*d)({ragged}{rows}) = ulcx_decode_crops_spectra_ragged_host;\n'
           'int (*e)(int, int, int *) = ulcx_window_subblocks;\n'
           'int f = ULCX_SPECTRA_LR;\n'
           'int main(void){return 0;}\n')
    p = subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-"],
                       input=src.encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()


# ---------------------------------------------------------------------------------------------------------------------
# ulcx_window_subblocks
# ---------------------------------------------------------------------------------------------------------------------
def _carried():
    """Every window code a block can carry (ulcDecoder.c:211-216): a first nybble without bit 3 and 1 above it, or a first nybble
    with bit 3 and any second nybble."""
    return [lo | 0x10 for lo in range(8)] + [lo | (hi << 4) for lo in range(8, 16) for hi in range(16)]


def test_window_subblocks_is_the_formats_table_and_the_oracles(lib):
    import ulc_amd
    lib.ulcx_window_subblocks.argtypes = [I, I, C.POINTER(C.c_int32)]
    codes = _carried()
    assert len(codes) == 8 + 128 and len(set(codes)) == len(codes)
    in_table = 0
    for bs in (256, 512, 1024, 2048, 4096, 8192, 16384, 32768):
        for wc in codes:
            sizes = (C.c_int32 * 4)(7, 7, 7, 7)
            n = lib.ulcx_window_subblocks(bs, wc, sizes)
            got = tuple(sizes[j] for j in range(n))
            assert 1 <= n <= 4 and got == S.subblocks_of(bs, wc), (bs, hex(wc), got)
            assert all(sizes[j] == 0 for j in range(n, 4)) and sum(got) == bs
            assert lib.ulcx_window_subblocks(bs, wc, None) == n
            assert ulc_amd.window_subblocks(bs, wc) == got
            if not wc & 8:
                assert got == (bs,)
            elif (wc >> 4) in _WINDOWS:                     # the format's own table (FormatSpecs.md), by divisor
                assert got == tuple(bs // d for d in _WINDOWS[wc >> 4]), (bs, hex(wc))
                in_table += 1
            else:                                           # second nybble 0 / 1: no row of the table; the reference decodes one full block
                assert (wc >> 4) in (0, 1) and got == (bs,)
    assert in_table == 8 * 8 * 14
    # codes no block can carry, and a bad BlockSize
    outside = [wc for wc in range(-3, 300) if wc not in set(codes)]
    assert 0 in outside and 0x20 in outside and 0x05 in outside and 256 in outside
    for wc in outside:
        sizes = (C.c_int32 * 4)(7, 7, 7, 7)
        assert lib.ulcx_window_subblocks(2048, wc, sizes) == 0, hex(wc)
    for bs in (0, -2048, 128, 3000, 65536):
        assert lib.ulcx_window_subblocks(bs, 0x10, None) == 0, bs
    assert ulc_amd.window_subblocks(2048, 0) == ()


# ---------------------------------------------------------------------------------------------------------------------
# refusals that need no device
# ---------------------------------------------------------------------------------------------------------------------
def test_refusals_without_a_device_come_in_order(lib):
    """No object, so every call is refused before anything touches a device; which argument the refusal names shows the order of
    the checks: the flags, NULL pointers, n, nFiles, nBlocks, the layout's scalars - and only then the missing decoder.  These are
    the crop calls' checks (tests/test_crops_capi.py, tests/test_crops_ragged_capi.py): the spectra entries run through them."""
    buf = (C.c_uint8 * 64)()
    n4 = (C.c_int32 * 4)()
    t8 = (C.c_int64 * 4)()
    co = (C.c_float * 16)()
    b, nn, tt, pc = C.addressof(buf), C.addressof(n4), C.addressof(t8), C.addressof(co)
    rows = [I, P, P, P, I, I, P, P, P]
    forms = []
    for name, head, tail in (("ulcx_decode_crops_spectra_dev", [P, I, P, LL, P, P, I, P], [P]), ("ulcx_decode_crops_spectra_host", [P, I, P, LL, P, P, I, P], []),
                             ("ulcx_decode_crops_spectra_ragged_dev", [P, I, P, LL, P, P, LL, P, P], [P]),
                             ("ulcx_decode_crops_spectra_ragged_host", [P, I, P, LL, P, P, LL, P, P], [])):
        fn = getattr(lib, name)
        fn.argtypes = head + rows + tail
        forms.append((name, fn, "ragged" in name, [None] * len(tail)))

    def call(fn, ragged, tail, nFiles=3, pay=b, nb=nn, idx=b, cnt=nn, n=2, file=nn, first=nn, count=None, nBlocks=2, flags=0, coef=pc, wc=nn, bits=nn,
             stride=64, istride=5, poffs=tt, ioffs=tt, ptotal=64, itotal=8):
        if ragged:
            return fn(None, nFiles, pay, ptotal, poffs, idx, itotal, ioffs, cnt, n, file, first, count, nBlocks, flags, coef, wc, bits, *tail)
        return fn(None, nFiles, pay, stride, nb, idx, istride, cnt, n, file, first, count, nBlocks, flags, coef, wc, bits, *tail)

    for name, fn, ragged, tail in forms:
        def refused(why, **kw):
            assert call(fn, ragged, tail, **kw) == ERR_ARG, (name, kw)
            msg = lib.ulcx_last_error().decode()
            assert msg.startswith(name + ":") and why in msg, (name, kw, msg)
        for flags in (2, 4, 3, -1, 1 << 16):                # an unknown flag bit, in front of everything else
            refused("flags", flags=flags)
            refused("flags", flags=flags, coef=None, n=0, nFiles=0, nBlocks=0)
        for lr in (0, 1):
            for k in ("pay", "idx", "cnt", "file", "first", "coef", "wc", "bits") + (("poffs", "ioffs") if ragged else ("nb",)):
                refused("NULL pointer", **{k: None}, flags=lr, n=0, nFiles=0, nBlocks=0)
            refused("(n 0)", flags=lr, n=0, nFiles=0, nBlocks=0)
            refused("(n -2)", flags=lr, n=-2)
            refused("(nFiles 0)", flags=lr, nFiles=0, nBlocks=0)
            refused("(nFiles -1)", flags=lr, nFiles=-1, nBlocks=99)
            refused("nBlocks is 1 .. maxBlocksPerCall - 1", flags=lr, nBlocks=0)
            refused("nBlocks is 1 .. maxBlocksPerCall - 1", flags=lr, nBlocks=-3)
            if ragged:
                refused("payloadTotal -1", flags=lr, ptotal=-1)
                refused("indexTotal -5", flags=lr, itotal=-5)
            else:
                refused("payloadStride 0", flags=lr, stride=0)
                refused("indexStride 0", flags=lr, istride=0)
            refused("no decoder", flags=lr)
            refused("no decoder", flags=lr, count=nn)
            refused("no decoder", flags=lr, coef=pc + 4)    # (a misaligned d_coef is an argument of a call that has an object: test_gpu_spectra.py)


# ---------------------------------------------------------------------------------------------------------------------
# the premises of the GPU tests' inputs
# ---------------------------------------------------------------------------------------------------------------------
def _census(bs, ch, q, sid):
    blocks, bits, _ = oracle_stream(bs, ch, q, sid)
    return S.census(f"oracle {bs}x{ch} q{q:g} id{sid}", blocks, bits, ch, bs)


def _covered(rows, K, n_blocks=S.N_BLOCKS):
    """Blocks of file f that some row (f, first) of n_blocks blocks has among its output blocks -> {f: set}."""
    out = {}
    for f, first in rows:
        out.setdefault(f, set()).update(range(first, min(first + n_blocks, K[f])))
    return out


def test_the_4096_stream_has_units_of_several_noise_passes():
    cen = _census(4096, 2, 30.0, 3)
    big = [(k, u["noise"]) for k, b in enumerate(cen) for u in b["units"] if u["noise"] > 2048]
    assert len(big) == 44 and max(n for _, n in big) == 3979
    rows = S.noise_pass_rows()
    cov = _covered(rows, S.geom_corpus((4096, 2)).K)
    assert {k for k, _ in big} <= cov[0], sorted({k for k, _ in big} - cov[0])


def test_the_streams_carry_full_blocks_every_decimation_pattern_tails_and_a_noiseless_block():
    seen = set()
    for bs, ch, q, sid in ORACLE_CASES:
        cen = _census(bs, ch, q, sid)
        shapes = {b["shape"] for b in cen}
        assert (1,) in shapes
        dec = shapes & S.DECIMATED
        seen |= dec
        if (bs, ch) == (4096, 2):
            assert dec == S.DECIMATED
        elif (bs, ch) == (1024, 1):
            assert len(dec) == 2
        else:
            assert dec == S.DECIMATED - {(4, 8, 8, 2)}
        blocks, bits, _ = oracle_stream(bs, ch, q, sid)
        tails = 0
        for k in range(blocks.shape[0]):
            kinds = {}
            S.decode_block_coefficients(blocks[k, :(int(bits[k]) + 7) // 8], ch, bs, kinds)
            tails += kinds.get("tail", 0)
        assert 15 <= tails <= 35, (bs, ch, tails)
        noiseless = [k for k, b in enumerate(cen) if all(u["noise"] == 0 for u in b["units"])]
        assert len(noiseless) == 1, (bs, ch, noiseless)
        # the rows of the row test reach every block of the oracle-encoded file (file 0 of its corpus): each shape, each tail, the noiseless one
        cor = S.geom_corpus((bs, ch))
        cov = _covered(S.seventy_rows(cor), cor.K)
        for f in range(cor.F):
            assert cov[f] == set(range(cor.K[f])), (bs, ch, f, sorted(set(range(cor.K[f])) - cov[f]))
    assert seen == S.DECIMATED


def test_a_unit_needs_a_fourth_round_of_record_fetches():
    """synth_unit fetches a unit's plain-run records 64 at a time and has the first three rounds in flight early: a unit of more
    than 192 records runs the loop's fourth round.  The last block of the 2048 x 3 stream has one (at least 207), and the row
    tests reach it (a row two blocks before the file's end)."""
    cen = _census(2048, 3, 60.0, 3)
    recs = [(u["records"], k) for k, b in enumerate(cen) for u in b["units"]]
    assert max(recs) == (207, 39)
    cor = S.geom_corpus((2048, 3))
    assert (0, 38) in S.row_table(cor) and 39 in _covered(S.row_table(cor), cor.K)[0]


def test_the_32768_files_reach_the_lds_ceiling_with_every_kind_of_unit():
    tr = S.big_stream(1, True)
    cen = S.census(tr.name, tr.blocks, tr.bits, 1, 32768)
    assert tr.K == 3 and max(u["noise"] for b in cen for u in b["units"]) == 15996
    assert all(b["shape"] != (1,) for b in cen for u in b["units"] if u["noise"] > 2048)
    st = S.big_stream(1, False)
    cen = S.census(st.name, st.blocks, st.bits, 1, 32768)
    full = [k for k, b in enumerate(cen) if b["shape"] == (1,) and any(u["noise"] > 0 and u["coded"] > 0 for u in b["units"])]
    assert full == [2], full                                # an un-decimated block of 32768 with coded and noise coefficients
    assert max(u["records"] for u in cen[2]["units"]) > 192 and max(u["noise"] for u in cen[2]["units"]) > 2048
    for f in (tr, st):                                      # 2 rows x 2 blocks from blocks 0 and 1 reach every block of a 3-block file
        assert _covered([(0, 0), (0, 1)], [f.K], 2)[0] == {0, 1, 2}
    pair = S.big_stream(2, True)
    assert pair.K == 3 and (pair.bits > 0).all() and (pair.coef[1:, 1] != 0).any()       # the in-place LR path's file: a side channel that is not silent


def test_expected_values_are_the_oracles_coefficients_channels_first():
    """The reference the GPU tests compare against: orc_decode_stream_coefs over the whole file, sliced and transposed; LR in
    float32; zeros where a row has no block.  Against the decoder written from the format's text where it can speak: magnitudes,
    and exact values of the coded coefficients."""
    cor = S.geom_corpus((2048, 2))
    f = cor.files[0]
    coef, wc, bits = f.expected_spec(37, 5)
    assert coef.shape == (2, 5, 2048) and (bits[:3] > 0).all() and (bits[3:] == 0).all() and (wc[3:] == 0).all() and not coef[:, 3:].any()
    for k in (1, 9, 24, 38):
        spec, noise, _ = S.decode_block_coefficients(f.blocks[k, :(int(f.bits[k]) + 7) // 8], 2, 2048)
        assert np.array_equal(np.abs(f.coef[k]), np.abs(spec)) and np.array_equal(f.coef[k][noise == 0], spec[noise == 0]), k
    lr = f.expected_spec(5, 5, lr=True)[0]
    m, s = f.coef[5:10, 0], f.coef[5:10, 1]
    assert S.same_bits(lr[0], m + s) and S.same_bits(lr[1], m - s) and not S.same_bits(lr[0], m)
    c3 = S.geom_corpus((2048, 3)).files[0]
    lr3 = c3.expected_spec(5, 5, lr=True)[0]
    assert S.same_bits(lr3[2], c3.coef[5:10, 2])            # a trailing single channel is untouched
    short = f.expected_spec(5, 5, count=2)
    assert (short[2][:2] > 0).all() and (short[2][2:] == 0).all() and not short[0][:, 2:].any()
