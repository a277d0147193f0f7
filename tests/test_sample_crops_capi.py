"""Sample crops (include/ulc_amd.h section 3: ulcx_crop_blocks / ulcx_decode_crops_samples_*) at the C-ABI boundary, without a
GPU: the block arithmetic against brute force, corpus.sample_rows (the numpy restatement of the prologue kernel) against the
same brute force, the header's declarations as C, and the refusals that need no device."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
LIB = os.path.join(ROOT, "ulc-codec_amd", "libulc_amd.so")
NAMES = ("ulcx_decode_crops_samples_dev", "ulcx_decode_crops_samples_dev_pcm16", "ulcx_decode_crops_samples_host",
         "ulcx_decode_crops_samples_ragged_dev", "ulcx_decode_crops_samples_ragged_dev_pcm16", "ulcx_decode_crops_samples_ragged_host")
BLOCK_SIZES = (256, 512, 1024, 2048, 4096, 8192, 16384, 32768)
ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ulc-codec_amd"), "-j8"], stdout=subprocess.DEVNULL)
    l = C.CDLL(LIB)
    l.ulcx_last_error.restype = C.c_char_p
    l.ulcx_crop_blocks.argtypes = [C.c_int, C.c_int]
    return l


def _touched(bs, n, skip):
    """Brute force for one start: blocks touched by samples skip .. skip + len - 1, for len = 0 .. n -> int64 [n + 1].  The samples
    are walked one by one: a sample opens a block when it is the first or its position is a multiple of bs."""
    j = np.arange(n, dtype=np.int64)
    opens = ((skip + j) % bs == 0) | (j == 0)
    return np.concatenate([[0], np.cumsum(opens)])


def _worst(bs, n):
    """The same walk for all bs starts abreast -> the most blocks any start touches, for len = 0 .. n.  Sample number j (from 0)
    of the crop that starts at `skip` sits at position skip + j: it opens a block for every start when j == 0, else for the one
    start with (skip + j) % bs == 0."""
    c = np.ones(bs, np.int64)                               # after the first sample
    worst = np.zeros(n + 1, np.int64)
    worst[1] = 1
    top = 1
    for j in range(1, n):
        k = (-j) % bs
        c[k] += 1
        top = max(top, int(c[k]))
        worst[j + 1] = top
    return worst


@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_crop_blocks_is_the_worst_case_over_every_start(lib, bs):
    n = 3 * bs + 2
    worst = _worst(bs, n)
    for sk in (0, 1, bs - 1):                               # (the abreast walk against the one-start walk)
        assert (_touched(bs, n, sk) <= worst).all() and (sk != bs - 1 or np.array_equal(_touched(bs, n, sk), worst))
    got = np.array([lib.ulcx_crop_blocks(bs, s) for s in range(1, n + 1)])
    assert np.array_equal(got, worst[1:]), (bs, np.flatnonzero(got != worst[1:])[:5])
    assert got[0] == 1 and got[1] == 2 and got[bs - 1] == 2 and got[bs] == 2 and got[bs + 1] == 3      # nSamples 1, 2, BS, BS + 1, BS + 2
    for bad in ((bs, 0), (bs, -1), (0, 5), (-bs, 5)):
        assert lib.ulcx_crop_blocks(*bad) == 0, bad


@pytest.mark.parametrize("bs", BLOCK_SIZES)
def test_sample_rows_restates_the_prologue(bs):
    import corpus
    n = 3 * bs + 2
    rng = np.random.default_rng(bs)
    skips = np.unique(np.concatenate([[0, 1, bs // 2, bs - 2, bs - 1], rng.integers(0, bs, 24)]))
    lens = np.arange(0, n + 1, dtype=np.int64)
    for base in (0, 7, (1 << 31) // bs + 3):               # block the start lies in; the last: positions past 2^31
        for sk in skips:
            start = np.full(lens.size, base * bs + int(sk), np.int64)
            first, count, skip = corpus.sample_rows(start, lens, bs)
            assert (first == base).all() and (skip == sk).all()
            want = _touched(bs, n, int(sk))
            assert np.array_equal(count, want), (bs, base, int(sk), np.flatnonzero(count != want)[:5])
    first, count, skip = corpus.sample_rows([-1, -bs, 0], [5, 5, 0], bs)
    assert first.tolist() == [-1, -1, 0] and count.tolist() == [0, 0, 0] and skip.tolist() == [0, 0, 0]


def test_sample_crop_entry_points_are_exported_and_bound(lib):
    import ulc_amd
    import corpus
    for n in NAMES + ("ulcx_crop_blocks",):
        assert hasattr(lib, n), n
        assert n in ulc_amd.EXPORTS, n
    for m in ("decode_crops_samples", "decode_crops_samples_dev", "decode_crops_samples_ragged", "decode_crops_samples_ragged_dev"):
        assert hasattr(ulc_amd.BatchDecoder, m), m
    assert hasattr(corpus.CropCorpus, "sample_crops") and hasattr(corpus, "sample_rows")
    assert ulc_amd.crop_blocks(2048, 30 * 2048 + 1) == 31


def test_header_declares_the_six_entries_with_these_types():
    strided = "ulcx_decoder *, int, const uint8_t *, long long, const int32_t *, const ulcx_index_entry *, int, const int32_t *,\n"
    ragged = ("ulcx_decoder *, int, const uint8_t *, long long, const int64_t *, const ulcx_index_entry *, long long, const int64_t *,\n"
              "         const int32_t *,\n")
    rows = "         int, const int32_t *, const int64_t *, const int32_t *, int, "
    src = ('#include "ulc_amd.h"\n'
           'int (*z)(int, int) = ulcx_crop_blocks;\n'
           f'int (*a)({strided}{rows}float *, int32_t *, void *) = ulcx_decode_crops_samples_dev;\n'
           f'int (*b)({strided}{rows}int16_t *, int32_t *, void *) = ulcx_decode_crops_samples_dev_pcm16;\n'
           f'int (*c)({strided}{rows}float *, int32_t *) = ulcx_decode_crops_samples_host;\n'
           f'int (*d)({ragged}{rows}float *, int32_t *, void *) = ulcx_decode_crops_samples_ragged_dev;\n'
           f'int (*e)({ragged}{rows}int16_t *, int32_t *, void *) = ulcx_decode_crops_samples_ragged_dev_pcm16;\n'
           f'int (*f)({ragged}{rows}float *, int32_t *) = ulcx_decode_crops_samples_ragged_host;\n'
           'int main(void){return 0;}\n')
    p = subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-"],
                       input=src.encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()


def test_refusals_without_a_device(lib):
    """No object: everything is refused before a device is touched, under the entry's own name; nSamples < 1 is refused first."""
    buf = (C.c_uint8 * 256)()
    p = C.addressof(buf)
    P, I, LL = C.c_void_p, C.c_int, C.c_longlong
    strided = [P, I, P, LL, P, P, I, P, I, P, P, P, I, P, P]
    ragged = [P, I, P, LL, P, P, LL, P, P, I, P, P, P, I, P, P]
    for name in NAMES:
        fn = getattr(lib, name)
        is_ragged, is_dev = "ragged" in name, "_dev" in name
        fn.argtypes = (ragged if is_ragged else strided) + ([P] if is_dev else [])
        fn.restype = I
        head = [None, 1, p, 1, p, p, 1, p, p] if is_ragged else [None, 1, p, 1, p, p, 1, p]
        tail = [p, p] + ([None] if is_dev else [])
        for n_samples, why in ((0, "nSamples 0"), (-3, "nSamples -3")):
            assert fn(*head, 1, p, p, p, n_samples, *tail) == ERR_ARG
            msg = lib.ulcx_last_error().decode()
            assert msg.startswith(name + ":") and why in msg, msg
        assert fn(*head, 1, p, None, p, 5, *tail) == ERR_ARG              # no d_start
        assert lib.ulcx_last_error().decode().startswith(name + ":") and "NULL" in lib.ulcx_last_error().decode()
        assert fn(*head, 0, p, p, p, 5, *tail) == ERR_ARG                 # n 0
        assert "n 0" in lib.ulcx_last_error().decode()
        assert fn(*head, 1, p, p, None, 5, *tail) == ERR_ARG              # a NULL d_len is allowed: the refusal is the missing object
        assert lib.ulcx_last_error().decode() == name + ": no decoder"
