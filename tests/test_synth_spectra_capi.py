"""Synthesis from spectra (include/ulc_amd.h section 3: ulcx_synth_spectra_*) at the C-ABI boundary, without a GPU: the three
entries' presence, and the premises of tests/test_gpu_synth_spectra.py's inputs - asserted here on the oracle and the float64
referee alone, nothing of the library under test: what the rows hold, the two-block dependence ULCX_SYNTH_WARM rests on, and that
the codes the GPU test plants as bad are exactly codes ulcx_window_subblocks rejects."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
import mdct_referee as R
import synth_spectra_testlib as Y
from seek_testlib import geometries

LIB = os.path.join(ROOT, "ulc-codec_amd", "libulc_amd.so")
NAMES = ("ulcx_synth_spectra_dev", "ulcx_synth_spectra_dev_pcm16", "ulcx_synth_spectra_host")
GEOMS = sorted(geometries().keys())
ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ulc-codec_amd"), "-j8"], stdout=subprocess.DEVNULL)
    l = C.CDLL(LIB)
    l.ulcx_last_error.restype = C.c_char_p
    return l


def test_synth_entry_points_are_exported_and_bound(lib):
    import ulc_amd
    import corpus
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in ulc_amd.EXPORTS, n
    for m in ("synth_spectra", "synth_spectra_dev"):
        assert hasattr(ulc_amd.BatchDecoder, m), m
    assert ulc_amd.SYNTH_WARM == 2 and ulc_amd.SPECTRA_LR == 1 and callable(corpus.synth_spectra)


def test_header_compiles_as_c_and_declares_the_calls():
    head = "ulcx_decoder *, int, int, int, const float *, const int32_t *, "
    src = ('#include "ulc_amd.h"\n'
           f'int (*a)({head}float *, int32_t *, void *) = ulcx_synth_spectra_dev;\n'
           f'int (*b)({head}int16_t *, int32_t *, void *) = ulcx_synth_spectra_dev_pcm16;\n'
           f'int (*c)({head}float *, int32_t *) = ulcx_synth_spectra_host;\n'
           'int f = ULCX_SYNTH_WARM | ULCX_SPECTRA_LR;\n'
           '_Static_assert(ULCX_SYNTH_WARM == 2 && (ULCX_SYNTH_WARM & ULCX_SPECTRA_LR) == 0, "flags");\n'
           'int main(void){return 0;}\n')
    p = subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-"],
                       input=src.encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()


def test_refusals_without_a_device(lib):
    """No object: every call is refused before anything touches a device - an unknown flag first, then a NULL pointer, then n."""
    P, I = C.c_void_p, C.c_int
    lib.ulcx_synth_spectra_dev.argtypes = [P, I, I, I, P, P, P, P, P]
    lib.ulcx_synth_spectra_host.argtypes = [P, I, I, I, P, P, P, P]
    buf = (C.c_float * 64)()
    a = C.addressof(buf)
    assert lib.ulcx_synth_spectra_dev(None, 1, 1, 4, a, a, a, a, None) == ERR_ARG and b"flags" in lib.ulcx_last_error()
    assert lib.ulcx_synth_spectra_dev(None, 1, 1, 0, None, a, a, a, None) == ERR_ARG and b"NULL" in lib.ulcx_last_error()
    assert lib.ulcx_synth_spectra_dev(None, 0, 1, 0, a, a, a, a, None) == ERR_ARG and b"n 0" in lib.ulcx_last_error()
    assert lib.ulcx_synth_spectra_dev(None, 1, 1, 0, a, a, a, a, None) == ERR_ARG and b"no decoder" in lib.ulcx_last_error()
    assert lib.ulcx_synth_spectra_host(None, 1, 1, 8, a, a, a, a) == ERR_ARG and b"flags" in lib.ulcx_last_error()
    assert lib.ulcx_synth_spectra_host(None, 1, 1, 3, a, a, a, a) == ERR_ARG and b"no decoder" in lib.ulcx_last_error()


# ---------------------------------------------------------------------------------------------------------------------
# premises of the GPU inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS)
def test_rows_hold_what_the_gpu_test_says(geom):
    """The WARM rows of a geometry contain a decimated block, an overlap clipped by the previous sub-block, and starts directly
    behind a window switch; some run past their stream's end; the rows without a plane in front end at every plane."""
    bs, ch = geom
    refs = Y.geom_streams(geom)
    rows = Y.warm_rows(refs)
    assert len(rows) == 70
    coef, wc, pcm, live = Y.stack(refs, rows, Y.N_OUT, 1)
    assert coef.shape == (70, ch, Y.N_OUT + 1, bs) and pcm.shape == (70, ch, Y.N_OUT * bs)
    decimated = clipped = behind_switch = 0
    for i, (s, first) in enumerate(rows):
        codes = [int(w) for w in wc[i] if w]
        decimated += any(len(Y.subblocks_of(bs, w)) > 1 for w in codes)
        clipped += any(ov > prev > 0 for ov, prev in Y.transitions_of(bs, codes))
        behind_switch += first in Y.switched(refs[s])
    assert decimated >= 10 and clipped >= 10 and behind_switch >= 3 * len(refs), (decimated, clipped, behind_switch)
    assert (live == 0).any() and (live.sum(axis=1) == Y.N_OUT).sum() >= 30 and (live.sum(axis=1) == 0).any()
    hc, hw, hp, hl = Y.head_rows(refs)
    assert {int(x) for x in hl.sum(axis=1)} == set(range(1, Y.N_OUT + 1)) and (hw[:, 0] != 0).all()


@pytest.mark.parametrize("geom", GEOMS)
def test_pcm_of_a_block_depends_on_two_planes(geom):
    """The referee's synthesis of the planes from k - 1 on reproduces the oracle's PCM of the blocks from k on within TOL, for
    starts directly behind window switches: the PCM of block k depends on the planes and codes of blocks k - 1 and k only - what
    ULCX_SYNTH_WARM rests on.  (Output block 0 of such a synthesis, which laps against nothing, is NOT the oracle's.)"""
    bs, ch = geom
    worst, off = 0.0, 0
    for ref in Y.geom_streams(geom):
        sw = Y.switched(ref)
        for k in (sw[0], sw[len(sw) // 2], sw[-1]):
            m = min(Y.N_OUT, ref.K - k)
            planes = Y.planes(ref)[:, k - 1:k + m].transpose(1, 0, 2).reshape(m + 1, ch * bs)
            headers = [Y.referee_header(w) for w in ref.wc[k - 1:k + m + 1]]
            y = R.synthesise(planes, headers, bs, ch)[:(m + 1) * bs]
            e = R.unit_errors(R.pcm_units(Y.pcm_planes(ref)[:, (k - 1) * bs:(k + m) * bs].T, bs), R.pcm_units(y, bs))
            worst = max(worst, e[1:].max())
            off += bool(e[0].max() > 100 * Y.TOL)
    assert worst <= Y.TOL, worst
    assert off >= 1                                        # the block that lacks its plane in front does differ
    print(f"{bs}x{ch}: worst {worst:.2e}")


def test_bad_codes_are_what_window_subblocks_rejects(lib):
    lib.ulcx_window_subblocks.argtypes = [C.c_int, C.c_int, C.c_void_p]
    assert 0 in Y.BAD_CODES and len(Y.BAD_CODES) == 6
    for bs in (256, 2048, 4096, 32768):
        for wc in Y.BAD_CODES:
            assert lib.ulcx_window_subblocks(bs, C.c_int(wc).value, None) == 0, hex(wc)
    # and every code the GPU inputs carry for a live block is accepted
    for geom in GEOMS:
        for ref in Y.geom_streams(geom):
            assert all(lib.ulcx_window_subblocks(ref.bs, int(w), None) > 0 for w in ref.wc), ref.name
    for bs, ch in ((256, 1), (2048, 2)):
        ref = Y.code_stream(bs, ch)
        assert all(lib.ulcx_window_subblocks(bs, int(w), None) > 0 for w in ref.wc)
    assert all(lib.ulcx_window_subblocks(256, int(w), None) > 0 for w in Y.referee_case(256, 6, 3)["wc"])
