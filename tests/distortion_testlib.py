"""The referee of the distortion tests (tests/test_distortion_capi.py, tests/test_gpu_distortion.py): what
ulcx_decode_crops_distortion_* must give, in numpy float64 and in the summation order include/ulc_amd.h defines - every term formed
from the float32 values with a separate multiplication and subtraction, the terms of a segment added by the pairwise tree over
adjacent elements.  Results are compared as uint64 views.  Corpora, rows and the oracle's coded coefficients are
spectra_testlib's, unchanged; here are the reference planes, the BlockSize 256 corpus (the one geometry whose nSeg 64 is
W = 4), and the cases the GPU tests name.  CPU only; nothing here runs the library under test."""
import functools
import numpy as np
import spectra_testlib as S
from ulc_testlib import same_bits64
from corpus_testlib import Corpus, oracle_file

N_BLOCKS = S.N_BLOCKS
INT32_MAX = 2 ** 31 - 1
SMALL = (256, 2)                                           # BlockSize 256: nSeg 64 leaves W = 4, the tree's levels inside a lane


def tree(t):
    """Pairwise sum over adjacent elements of the last axis (a power of two long), down to one value."""
    t = np.asarray(t, np.float64)
    while t.shape[-1] > 1:
        t = t[..., 0::2] + t[..., 1::2]
    return t[..., 0]


def terms(ref, y):
    """float32 planes [..., bs] -> the three terms per element, float64 [..., bs] each: r * r, y * y, (r - y) * (r - y)."""
    r, y = np.asarray(ref, np.float32).astype(np.float64), np.asarray(y, np.float32).astype(np.float64)
    d = r - y
    return r * r, y * y, d * d


def sums(ref, y, n_seg):
    """ref, y float32 [..., bs] -> float64 [..., n_seg, 3] = {S, Y, E} per segment of bs / n_seg elements."""
    with np.errstate(all="ignore"):
        out = [tree(t.reshape(t.shape[:-1] + (n_seg, t.shape[-1] // n_seg))) for t in terms(ref, y)]
    return np.stack(out, axis=-1)


def halve(dist):
    """dist [..., n_seg, 3] -> [..., n_seg / 2, 3]: adjacent segments added, one tree level up."""
    with np.errstate(all="ignore"):
        return dist[..., 0::2, :] + dist[..., 1::2, :]


def first_diff(a, b):
    """Where two float64 arrays differ in bits (the first few indices), for messages."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return f"shapes {a.shape} vs {b.shape}"
    w = np.argwhere(a.view(np.uint64) != b.view(np.uint64))[:3]
    return [(tuple(int(v) for v in i), float(a[tuple(i)]), float(b[tuple(i)])) for i in w]


def ref_planes(n_ref, ch, n_ref_blocks, bs, seed=7):
    """Seeded float32 reference planes [n_ref][ch][n_ref_blocks][bs]: values of very different exponent (2^-60 .. 2^20, where the
    coded coefficients are of order 1), and, spread over every plane, float32 denormals, +0 and -0."""
    rng = np.random.default_rng(seed)
    shape = (n_ref, ch, n_ref_blocks, bs)
    v = (rng.standard_normal(shape) * np.exp2(rng.integers(-60, 21, shape))).astype(np.float32)
    kind = rng.integers(0, 16, shape)
    den = (rng.integers(1, 1 << 23, shape).astype(np.uint32) | (rng.integers(0, 2, shape).astype(np.uint32) << 31)).view(np.float32)
    v = np.where(kind == 0, den, v)
    v = np.where(kind == 1, np.float32(0.0), v)
    v = np.where(kind == 2, np.float32(-0.0), v)
    return np.ascontiguousarray(v, np.float32)


def is_denormal(v):
    b = np.ascontiguousarray(v, np.float32).view(np.uint32)
    return ((b & 0x7F800000) == 0) & ((b & 0x007FFFFF) != 0)


@functools.lru_cache(maxsize=None)
def small_corpus():
    """A BlockSize 256 stereo corpus of one oracle-encoded transient file (corpus_testlib.Corpus); signal 11: two window-switched
    blocks, of two patterns, which row_table() asks of a file."""
    return Corpus([oracle_file(*SMALL, 50.0, 11)])


def corpus_of(geom):
    """spectra_testlib.geom_corpus() for its geometries, and the BlockSize 256 corpus."""
    return small_corpus() if tuple(geom) == SMALL else S.geom_corpus(tuple(geom))


def geoms():
    from seek_testlib import geometries
    return sorted(geometries().keys()) + [SMALL]


def expected(coef, ref, ref_row, ref_first, n_seg):
    """coef float32 [n][ch][N][bs] (what the spectra call writes: zeros where a block is not live), live bool [n][N] taken from it by
    the caller -> the referee's sums against ref [n_ref][ch][n_ref_blocks][bs] (or None) under the absent-reference rule, float64
    [n][ch][N][n_seg][3].  ref_row / ref_first: sequences of n ints, or None."""
    n, ch, N, bs = coef.shape
    r = np.zeros((n, ch, N, bs), np.float32)
    if ref is not None:
        n_ref, _, n_rb, _ = ref.shape
        for i in range(n):
            row = i if ref_row is None else int(ref_row[i])
            if not 0 <= row < n_ref:
                continue
            for k in range(N):
                rb = (0 if ref_first is None else int(ref_first[i])) + k
                if 0 <= rb < n_rb:
                    r[i, :, k] = ref[row, :, rb]
    return sums(r, coef, n_seg), r


def expected_rows(cor, files, first, N, n_seg, ref=None, ref_row=None, ref_first=None, count=None, lr=False):
    """The whole expectation of a call on an undamaged corpus -> (dist [n][ch][N][n_seg][3], wc [n][N], bits [n][N]): the oracle's
    coefficients of the rows, the referee's sums of them against the reference, and +0.0 in all three sums of a block that is not
    live (its reference is not read)."""
    coef, wc, bits = cor.expected_spec(files, first, N, count, lr=lr)
    dist, _ = expected(coef, ref, ref_row, ref_first, n_seg)
    dist[np.broadcast_to((wc == 0)[:, None, :], dist.shape[:3])] = 0.0
    return dist, wc, bits


def absent_tables(n, n_ref, n_ref_blocks, N=N_BLOCKS):
    """The d_refRow / d_refFirst tables of the absent-reference test, n rows each: rows outside the reference (-1, n_ref,
    INT32_MAX) among valid ones that several crop rows share, and first blocks that leave no, some or all of a row's N blocks
    outside [0, n_ref_blocks) - negative ones, and ones near INT32_MAX whose sum with the block number needs 64 bits."""
    assert n_ref_blocks >= N + 2
    rows = [0, -1, 1 % n_ref, n_ref, 0, INT32_MAX, n_ref - 1, -INT32_MAX - 1]
    firsts = [0, 2, -2, n_ref_blocks - 2, -N, n_ref_blocks, INT32_MAX - 1, INT32_MAX, -INT32_MAX - 1, n_ref_blocks - N, -1]
    ref_row = [rows[i % len(rows)] for i in range(n)]
    ref_first = [firsts[(i // 2) % len(firsts)] for i in range(n)]
    return ref_row, ref_first


def outside(ref_row, ref_first, n_ref, n_ref_blocks, N=N_BLOCKS):
    """bool [n][N]: the blocks of the rows whose reference is absent under those tables (Python integers: no wrap)."""
    out = np.zeros((len(ref_row), N), bool)
    for i, (r, f) in enumerate(zip(ref_row, ref_first)):
        for k in range(N):
            out[i, k] = not (0 <= int(r) < n_ref and 0 <= int(f) + k < n_ref_blocks)
    return out
