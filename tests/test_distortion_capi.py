"""Distortion (include/ulc_amd.h section 3: ulcx_decode_crops_distortion_*) without a GPU: the four entries and their bindings, the
refusals that need no device, the referee's summation tree (tests/distortion_testlib.py) - its nesting and its distance from the
exact sum -, corpus.rung_plan on hand-made tensors, and a census of what the cases of tests/test_gpu_distortion.py hold."""
import ctypes as C
import math
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
import distortion_testlib as T
import spectra_testlib as S
from seek_testlib import oracle_stream

LIB = os.path.join(ROOT, "ulc-codec_amd", "libulc_amd.so")
NAMES = ("ulcx_decode_crops_distortion_dev", "ulcx_decode_crops_distortion_host", "ulcx_decode_crops_distortion_ragged_dev",
         "ulcx_decode_crops_distortion_ragged_host")
ERR_ARG = -1
P, I, LL = C.c_void_p, C.c_int, C.c_longlong
N = T.N_BLOCKS


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ulc-codec_amd"), "-j8"], stdout=subprocess.DEVNULL)
    l = C.CDLL(LIB)
    l.ulcx_last_error.restype = C.c_char_p
    return l


# ---------------------------------------------------------------------------------------------------------------------
# the entries
# ---------------------------------------------------------------------------------------------------------------------
def test_distortion_entry_points_are_exported_and_bound(lib):
    import ulc_amd
    import corpus
    l = ulc_amd.lib()
    for n in NAMES:
        assert hasattr(lib, n), n
        assert n in ulc_amd.EXPORTS, n
    # the spectra calls' arguments up to nBlocks, then d_ref, nRef, nRefBlocks, d_refRow, d_refFirst, nSeg, flags, d_dist, d_wc, d_bits
    rows_dev = [P, I, I, P, P, I, I, P, P, P]
    f32, i32, f64 = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_double)
    rows_host = [f32, I, I, i32, i32, I, I, f64, i32, i32]
    for name, spectra, head in (("ulcx_decode_crops_distortion_dev", "ulcx_decode_crops_spectra_dev", 13),
                                ("ulcx_decode_crops_distortion_ragged_dev", "ulcx_decode_crops_spectra_ragged_dev", 14)):
        assert getattr(l, name).argtypes == getattr(l, spectra).argtypes[:head] + rows_dev + [P], name
    for name, spectra, head in (("ulcx_decode_crops_distortion_host", "ulcx_decode_crops_spectra_host", 13),
                                ("ulcx_decode_crops_distortion_ragged_host", "ulcx_decode_crops_spectra_ragged_host", 14)):
        assert getattr(l, name).argtypes == getattr(l, spectra).argtypes[:head] + rows_host, name
    for m in ("decode_crops_distortion", "decode_crops_distortion_dev", "decode_crops_distortion_ragged", "decode_crops_distortion_ragged_dev"):
        assert hasattr(ulc_amd.BatchDecoder, m), m
    assert hasattr(corpus.CropCorpus, "distortion") and callable(corpus.rung_plan)


def test_header_compiles_as_c_and_declares_the_calls():
    rows = ('int, const int32_t *, const int32_t *, const int32_t *, int, const float *, int, int, const int32_t *, const int32_t *, int, int, '
            'double *, int32_t *, int32_t *')
    strided = 'ulcx_decoder *, int, const uint8_t *, long long, const int32_t *, const ulcx_index_entry *, int, const int32_t *, '
    ragged = 'ulcx_decoder *, int, const uint8_t *, long long, const int64_t *, const ulcx_index_entry *, long long, const int64_t *, const int32_t *, '
    src = ('#include "ulc_amd.h"\n'
           f'int (*a)({strided}{rows}, void *) = ulcx_decode_crops_distortion_dev;\n'
           f'int (*b)({strided}{rows}) = ulcx_decode_crops_distortion_host;\n'
           f'int (*c)({ragged}{rows}, void *) = ulcx_decode_crops_distortion_ragged_dev;\n'
           f'int (*d)({ragged}{rows}) = ulcx_decode_crops_distortion_ragged_host;\n'
           'int main(void){return 0;}\n')
    p = subprocess.run(["gcc", "-x", "c", "-std=c11", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-"],
                       input=src.encode(), capture_output=True)
    assert p.returncode == 0, p.stderr.decode()


def test_refusals_without_a_device_come_in_the_spectra_calls_order(lib):
    """No object: every call is refused before anything touches a device, and the refusal names what the spectra call would name -
    the flags first, NULL pointers (d_dist and d_wc among them; d_ref, d_refRow, d_refFirst and d_count may be NULL), n, nFiles,
    nBlocks, the layout's scalars, and only then the missing decoder.  What needs the object's BlockSize - nSeg, LR at 32768 - and
    the alignments are refusals of a call that has one (tests/test_gpu_distortion.py)."""
    buf = (C.c_uint8 * 64)()
    n4 = (C.c_int32 * 4)()
    t8 = (C.c_int64 * 4)()
    co = (C.c_float * 16)()
    dd = (C.c_double * 16)()
    b, nn, tt, pc, pd = C.addressof(buf), C.addressof(n4), C.addressof(t8), C.addressof(co), C.addressof(dd)
    rows = [I, P, P, P, I, P, I, I, P, P, I, I, P, P, P]
    forms = []
    for name, head, tail in ((NAMES[0], [P, I, P, LL, P, P, I, P], [P]), (NAMES[1], [P, I, P, LL, P, P, I, P], []),
                             (NAMES[2], [P, I, P, LL, P, P, LL, P, P], [P]), (NAMES[3], [P, I, P, LL, P, P, LL, P, P], [])):
        fn = getattr(lib, name)
        fn.argtypes = head + rows + tail
        forms.append((name, fn, "ragged" in name, [None] * len(tail)))

    def call(fn, ragged, tail, nFiles=3, pay=b, nb=nn, idx=b, cnt=nn, n=2, file=nn, first=nn, count=None, nBlocks=2, ref=pc, nRef=1, nRefBlocks=1,
             refRow=None, refFirst=None, nSeg=1, flags=0, dist=pd, wc=nn, bits=nn, stride=64, istride=5, poffs=tt, ioffs=tt, ptotal=64, itotal=8):
        rest = (n, file, first, count, nBlocks, ref, nRef, nRefBlocks, refRow, refFirst, nSeg, flags, dist, wc, bits, *tail)
        if ragged:
            return fn(None, nFiles, pay, ptotal, poffs, idx, itotal, ioffs, cnt, *rest)
        return fn(None, nFiles, pay, stride, nb, idx, istride, cnt, *rest)

    for name, fn, ragged, tail in forms:
        def refused(why, **kw):
            assert call(fn, ragged, tail, **kw) == ERR_ARG, (name, kw)
            msg = lib.ulcx_last_error().decode()
            assert msg.startswith(name + ":") and why in msg, (name, kw, msg)
        for flags in (2, 4, 3, -1, 1 << 16):
            refused("flags", flags=flags)
            refused("flags", flags=flags, dist=None, n=0, nFiles=0, nBlocks=0, nSeg=3)
        for lr in (0, 1):
            for k in ("pay", "idx", "cnt", "file", "first", "dist", "wc", "bits") + (("poffs", "ioffs") if ragged else ("nb",)):
                refused("NULL pointer", **{k: None}, flags=lr, n=0, nFiles=0, nBlocks=0)
            refused("(n 0)", flags=lr, n=0, nFiles=0, nBlocks=0)
            refused("(nFiles 0)", flags=lr, nFiles=0, nBlocks=0)
            refused("nBlocks is 1 .. maxBlocksPerCall - 1", flags=lr, nBlocks=0)
            if ragged:
                refused("payloadTotal -1", flags=lr, ptotal=-1)
            else:
                refused("payloadStride 0", flags=lr, stride=0)
            refused("no decoder", flags=lr)
            refused("no decoder", flags=lr, ref=None, nRef=0, nRefBlocks=0)
            refused("no decoder", flags=lr, refRow=nn, refFirst=nn, count=nn, nSeg=3)


# ---------------------------------------------------------------------------------------------------------------------
# the referee's tree
# ---------------------------------------------------------------------------------------------------------------------
def _planes(bs, seed):
    rng = np.random.default_rng(seed)
    y = (rng.standard_normal((3, bs)) * np.exp2(rng.integers(-12, 3, (3, bs)))).astype(np.float32)
    return T.ref_planes(1, 3, 1, bs, seed)[0, :, 0], y


@pytest.mark.parametrize("bs", [256, 2048, 32768])
def test_the_tree_nests_from_64_segments_down_to_the_block(bs):
    ref, y = _planes(bs, bs)
    d = T.sums(ref, y, 64)
    assert d.shape == (3, 64, 3) and (d[..., 0] > 0).all() and (d[..., 2] > 0).all()
    n_seg = 64
    while n_seg > 1:
        n_seg //= 2
        d = T.halve(d)
        assert T.same_bits64(d, T.sums(ref, y, n_seg)), n_seg


def test_the_tree_is_not_the_left_to_right_sum():
    y = np.random.default_rng(1).random(4096).astype(np.float32)
    seq = 0.0
    for t in T.terms(y, y)[1].tolist():
        seq = seq + t
    assert seq != T.sums(y, y, 1)[0, 1] and abs(seq - T.sums(y, y, 1)[0, 1]) < 1e-9 * seq


@pytest.mark.parametrize("bs,n_seg", [(256, 64), (256, 1), (2048, 8), (4096, 1), (32768, 1), (32768, 64)])
def test_the_tree_stays_within_its_bound_of_the_exact_sum(bs, n_seg):
    """A pairwise tree of W non-negative terms has log2(W) levels, each adding at most one rounding of 2^-53 relative to a partial
    sum that no later level shrinks: |tree - exact| <= log2(W) * 2^-53 * exact to first order.  Asserted with a factor 2 of slack
    against math.fsum of the same terms, which is exactly rounded."""
    ref, y = _planes(bs, 3 * bs + n_seg)
    W = bs // n_seg
    got = T.sums(ref, y, n_seg)
    tm = np.stack(T.terms(ref, y), -1).reshape(3, n_seg, W, 3)
    bound = 2 * math.log2(W) * 2.0 ** -53
    for c in range(3):
        for g in range(0, n_seg, max(1, n_seg // 8)):
            for j in range(3):
                exact = math.fsum(tm[c, g, :, j].tolist())
                assert abs(got[c, g, j] - exact) <= bound * exact, (c, g, j, got[c, g, j], exact)


def test_the_terms_keep_denormals_and_signed_zeros_as_values():
    den = np.array([1e-45, -3e-42, 0.0, -0.0], np.float32)
    assert T.is_denormal(den).tolist() == [True, True, False, False]
    s, yy, e = T.terms(den, np.zeros(4, np.float32))
    assert s[0] > 0 and s[1] > 0 and e[0] == s[0] and not np.signbit(s[2:]).any() and not np.signbit(e[2:]).any()
    assert T.same_bits64(T.sums(np.zeros(8, np.float32), den.repeat(2), 2)[..., 0], np.zeros(2))


# ---------------------------------------------------------------------------------------------------------------------
# corpus.rung_plan
# ---------------------------------------------------------------------------------------------------------------------
def _dist(snr_db, ch=2, seg=4):
    """snr_db [rung][clip][block] (inf: E = 0; -inf: S = 0 with E > 0) -> a distortion tensor with that block SNR, spread unevenly
    over channels and segments."""
    import torch
    snr = np.asarray(snr_db, np.float64)
    d = np.zeros(snr.shape[:2] + (ch,) + snr.shape[2:] + (seg, 3))
    w = np.arange(1, ch * seg + 1, dtype=np.float64).reshape(ch, 1, seg)
    for r in range(snr.shape[0]):
        for c in range(snr.shape[1]):
            for k in range(snr.shape[2]):
                v = snr[r, c, k]
                S_, E_ = (0.0, 1.0) if v == -np.inf else (1.0, 0.0) if v == np.inf else (1.0, 10.0 ** (-v / 10.0))
                d[r, c, :, k, :, 0] = S_ * w[:, 0] / w.sum()
                d[r, c, :, k, :, 2] = E_ * w[:, 0][::-1] / w.sum()
                d[r, c, :, k, :, 1] = 0.5
    return torch.from_numpy(d)


def test_rung_plan_takes_the_first_rung_that_reaches_the_target_and_merges_runs():
    import corpus
    inf = np.inf
    snr = [  # rung 0 (cheapest), rung 1, rung 2; 3 clips x 6 blocks
        [[30, 30, 10, 10, 30, 5], [5, 5, 5, 5, 5, 5], [inf, -inf, 21, 19.9, 20.1, 30]],
        [[40, 40, 25, 15, 40, 12], [25, 8, 8, 25, 25, 8], [inf, 30, 30, 30, 30, 30]],
        [[50, 50, 50, 18, 50, 14], [30, 9, 30, 30, 30, 9], [inf, inf, 40, 40, 40, 40]],
    ]
    d = _dist(snr)
    plan = corpus.rung_plan(d, [6, 6, 6], 20.0)
    assert plan[0] == [(0, 2), (1, 1), (2, 1), (0, 1), (2, 1)]             # first rung reaching 20 dB; none does: the last rung
    assert plan[1] == [(1, 1), (2, 2), (1, 2), (2, 1)]                     # fallback to the last rung, merged with its neighbour
    assert plan[2] == [(0, 1), (1, 1), (0, 1), (1, 1), (0, 2)]             # E = 0: +inf reaches; S = 0 with E > 0: -inf does not
    # blocks shorter than the tensor, a clip of no blocks, and a list of per-rung tensors in place of one tensor
    short = corpus.rung_plan([d[0], d[1], d[2]], [3, 0, 1], 20.0)
    assert short == [[(0, 2), (1, 1)], [], [(0, 1)]]
    assert corpus.rung_plan(d, [9, 6, 6], 20.0)[0] == plan[0]              # a count past the tensor plans what the tensor holds
    # one rung: every block is that rung
    assert corpus.rung_plan(d[:1], [6, 6, 6], 99.0) == [[(0, 6)]] * 3
    # the target is reached at equality
    import torch
    exact = torch.zeros((2, 1, 1, 2, 1, 3), dtype=torch.float64)
    exact[0, ..., 0], exact[0, ..., 2] = 100.0, 1.0                        # 10 log10(100) is 20 exactly
    exact[1, ..., 0], exact[1, ..., 2] = 1000.0, 1.0
    assert corpus.rung_plan(exact, [2], 20.0) == [[(0, 2)]] and corpus.rung_plan(exact, [2], 20.5) == [[(1, 2)]]
    with pytest.raises(corpus.UlcError):
        corpus.rung_plan(d[0], [6, 6, 6], 20.0)
    with pytest.raises(corpus.UlcError):
        corpus.rung_plan(d, [6, 6], 20.0)


def test_rung_plan_gives_what_switch_takes():
    """CropCorpus.switch() on a stand-in that records what it hands splice(): every run becomes one segment (file_of(rung, clip),
    position, n_blocks), the positions running on through the clip."""
    import corpus

    class Ladder:
        n_clips = 2
        file_of = lambda self, rung, clip: rung * self.n_clips + clip
        splice = lambda self, dec, segments: (segments, None)

    d = _dist([[[30, 10, 10, 30]] * 2, [[40, 40, 40, 40]] * 2])
    plan = corpus.rung_plan(d, [4, 3], 20.0)
    assert plan == [[(0, 1), (1, 2), (0, 1)], [(0, 1), (1, 2)]]
    assert all(isinstance(r, int) and isinstance(nb, int) for row in plan for r, nb in row)
    segs = corpus.CropCorpus.switch(Ladder(), None, plan)
    assert segs == [[(0, 0, 1), (2, 1, 2), (0, 3, 1)], [(1, 0, 1), (3, 1, 2)]]
    assert [sum(nb for _, nb in row) for row in plan] == [4, 3]


# ---------------------------------------------------------------------------------------------------------------------
# what the GPU cases hold
# ---------------------------------------------------------------------------------------------------------------------
def _covered(rows, K, n_blocks=N):
    out = {}
    for f, first in rows:
        out.setdefault(f, set()).update(range(first, min(first + n_blocks, K[f])))
    return out


def test_census_of_the_gpu_cases():
    # rows with dead blocks: in every geometry the seventy rows run past a file's end and start at its end
    for geom in T.geoms():
        cor = T.corpus_of(geom)
        rows = S.seventy_rows(cor)
        _, wc, bits = cor.expected_spec([f for f, _ in rows], [k for _, k in rows], N)
        dead = wc == 0
        assert dead.any(axis=1).sum() >= 3 and dead.all(axis=1).any() and (~dead).all(axis=1).any(), geom
        assert ((bits == 0) == dead).all()
    # a decimated block of each of the four patterns, under the rows of the 4096 x 2 corpus
    bs, ch = 4096, 2
    blocks, bits, _ = oracle_stream(bs, ch, 30.0, 3)
    cen = S.census(f"oracle {bs}x{ch} q30 id3", blocks, bits, ch, bs)
    cor = S.geom_corpus((bs, ch))
    cov = _covered(S.seventy_rows(cor), cor.K)[0]
    assert {cen[k]["shape"] for k in cov} >= S.DECIMATED
    # a unit of more than 2048 noise coefficients, under the noise rows
    big = {k for k, b in enumerate(cen) for u in b["units"] if u["noise"] > 2048}
    assert big and big <= _covered(S.noise_pass_rows(), cor.K)[0]
    # the BlockSize 256 corpus: a decimated block too, and its nSeg 64 is W = 4
    small = T.small_corpus()
    assert small.bs // 64 == 4 and sum(1 for w in small.files[0].wc if int(w) & 8) >= 2
    # denormal reference values, signed zeros and a wide range of exponents in every plane
    ref = T.ref_planes(3, 2, N + 2, 256)
    for plane in ref.reshape(-1, 256):
        assert T.is_denormal(plane).sum() >= 4 and (plane == 0).sum() >= 4 and np.signbit(plane[plane == 0]).any()
        e = np.frexp(plane[(plane != 0) & ~T.is_denormal(plane)])[1]
        assert e.max() - e.min() > 40
    # reference rows and blocks out of range: some, all and no block of a row; sums that need 64 bits
    n_ref, n_rb = 3, N + 2
    row, first = T.absent_tables(70, n_ref, n_rb)
    out = T.outside(row, first, n_ref, n_rb)
    valid = np.array([0 <= r < n_ref for r in row])
    assert {-1, n_ref, T.INT32_MAX} <= set(row) and valid.sum() >= 30
    per_row = out[valid].sum(axis=1)
    assert (per_row == 0).any() and (per_row == N).any() and ((per_row > 0) & (per_row < N)).any()
    assert any(f < 0 for f in first)
    wraps = [f for f in first if f <= T.INT32_MAX < f + N - 1]      # first + k leaves int32: formed in 32 bits it would turn negative
    assert wraps and all(out[i].all() for i, f in enumerate(first) if f in wraps)
    shared = [r for r in set(row) if 0 <= r < n_ref and row.count(r) >= 2]
    assert shared, "several crop rows name one reference row"
