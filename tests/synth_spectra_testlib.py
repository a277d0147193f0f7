"""Inputs and references of the synth-spectra tests (tests/test_synth_spectra_capi.py, tests/test_gpu_synth_spectra.py): what
ulcx_synth_spectra_* must give for planes a decoder holds.  Planes, window codes and PCM of a stream all come from ONE oracle run
(orc_decode_stream_coefs: both sides of the function under test), re-laid as the call takes and writes them - planes
[C][K][bs], PCM [C][K * bs]; arbitrary planes are checked against the float64 referee (tests/mdct_referee.py).  CPU only; nothing
here runs the library under test."""
import functools
import numpy as np
import mdct_referee as R
from ulc_testlib import spec_stream, same_bits, to_pcm16
from seek_testlib import oracle_pcm
from corpus_testlib import File, geom_files
from spectra_testlib import subblocks_of, big_stream
from test_transform_referee import ALL_CODES, TOL, all_codes_sequence

SPECTRA_LR, SYNTH_WARM = 1, 2
N_OUT = 5                                                  # output blocks per row of the row tests
# what the GPU test plants for a window code: the spectra calls' "not live", and int32s no block can carry
BAD_CODES = (0, 0x05, 0x25, 0x100, -1, 0x7FFFFFFF)
POISON_F, POISON_I16, POISON_I32 = np.float32(7.25), np.int16(0x5A5A), np.int32(0x5A5A5A5A)


@functools.lru_cache(maxsize=None)
def planes(f):
    """A corpus_testlib.File's coefficients as the call takes them: [C][K][bs]."""
    assert (f.obits > 0).all(), f.name
    return np.ascontiguousarray(f.coef.transpose(1, 0, 2))


@functools.lru_cache(maxsize=None)
def pcm_planes(f):
    """A File's sequential decode as the call writes it: [C][K * bs]."""
    return np.ascontiguousarray(f.pcm.reshape(f.K * f.bs, f.ch).T)


def row(f, first, n_out, warm):
    """-> (coef [C][nPl][bs], wc [nPl], pcm [C][n_out * bs], live [n_out]) of the row of File f whose output starts at block `first`:
    planes first - warm .. first + n_out - 1, zeros with code 0 past the stream's end; the PCM of the sequential decode."""
    assert first - warm >= 0
    n_pl = n_out + warm
    coef, wc = np.zeros((f.ch, n_pl, f.bs), np.float32), np.zeros(n_pl, np.int32)
    pcm, live = np.zeros((f.ch, n_out * f.bs), np.float32), np.zeros(n_out, np.int32)
    p0 = first - warm
    m = max(0, min(n_pl, f.K - p0))
    coef[:, :m], wc[:m] = planes(f)[:, p0:p0 + m], f.wc[p0:p0 + m]
    mo = max(0, min(n_out, f.K - first))
    pcm[:, :mo * f.bs] = pcm_planes(f)[:, first * f.bs:(first + mo) * f.bs]
    live[:mo] = 1
    return coef, wc, pcm, live


@functools.lru_cache(maxsize=None)
def geom_streams(geom):
    """The oracle-encoded and hand-assembled streams of a geometry of seek_testlib.geometries()."""
    return geom_files(geom)


@functools.lru_cache(maxsize=None)
def code_stream(bs, ch, seed=7):
    """A hand-assembled stream (ulc_testlib.spec_stream) over every header code of test_transform_referee.ALL_CODES in a seeded
    order, behind one plain block."""
    headers = all_codes_sequence(seed, lead=[0])
    blocks, coefs, _ = spec_stream(headers, ch, bs, seed)
    ref = File(f"every header code {bs}x{ch}", bs, ch, blocks, oracle_pcm(blocks, ch, bs)[1])
    assert np.array_equal(ref.coef, coefs.reshape(ref.K, ch, bs))
    assert {int(w) if w & 8 else int(w) & 7 for w in ref.wc} == set(ALL_CODES)
    return ref


@functools.lru_cache(maxsize=None)
def big_ref():
    """Three blocks at 32768 x 1 (spectra_testlib.big_stream, with transients)."""
    return big_stream(1, True)


def switched(ref):
    """Output starts directly behind a window-switched block."""
    return [k + 1 for k in range(ref.K - 1) if int(ref.wc[k]) != 0x10]


def warm_rows(refs, n_out=N_OUT, total=70, seed=5):
    """(stream, first) of `total` WARM rows over the streams of a geometry: first 1, starts directly behind window-switched blocks,
    rows that run past the stream's end (their planes' codes end in 0), first = the last block, then seeded starts."""
    rows = []
    for s, ref in enumerate(refs):
        sw = switched(ref)
        assert len(sw) >= 2, ref.name
        rows += [(s, 1), (s, sw[0]), (s, sw[len(sw) // 2]), (s, sw[-1]), (s, ref.K - 2), (s, ref.K - 1), (s, ref.K)]
    rng = np.random.default_rng(seed)
    while len(rows) < total:
        s = int(rng.integers(0, len(refs)))
        rows.append((s, int(rng.integers(1, refs[s].K + 1))))
    return rows[:total]


def stack(refs, rows, n_out, warm):
    """-> (coef [n][C][nPl][bs], wc [n][nPl], pcm [n][C][n_out * bs], live [n][n_out]) of (stream, first) rows."""
    parts = [row(refs[s], first, n_out, warm) for s, first in rows]
    return tuple(np.stack([p[i] for p in parts]) for i in range(4))


def head_rows(refs, n_out=N_OUT, total=70):
    """Rows WITHOUT the plane in front: every stream from its block 0, again and again with the codes cut to 0 from plane
    t = n_out, n_out - 1, ..., 1 on (a file's end inside the row) -> (coef, wc, pcm, live) as stack()."""
    coef, wc, pcm, live = [], [], [], []
    i = 0
    while len(coef) < total:
        ref = refs[i % len(refs)]
        t = n_out - (i // len(refs)) % n_out
        c, w, p, l = row(ref, 0, n_out, 0)
        c, w, p, l = c.copy(), w.copy(), p.copy(), l.copy()
        w[t:] = 0; p[:, t * ref.bs:] = 0; l[t:] = 0        # (the planes behind stay: a dead block's coefficients are not looked at)
        coef.append(c); wc.append(w); pcm.append(p); live.append(l)
        i += 1
    return np.stack(coef), np.stack(wc), np.stack(pcm), np.stack(live)


def transitions_of(bs, wcs):
    """(nominal overlap, previous sub-block size) of every sub-block of a code sequence, by the oracle's pattern table
    (ulcDecoder.c:219-245): the overlap the decoder uses is the smaller of the two."""
    from ulc_testlib import oracle
    out, prev = [], 0
    for wc in wcs:
        pat = int(oracle().orc_decimation_pattern(int(wc)))
        while True:
            S = bs >> (pat & 7)
            out.append(((S >> (int(wc) & 7)) if pat & 8 else S, prev))
            prev = S
            pat >>= 4
            if S == bs or not pat:
                break
    return out


def referee_header(wc):
    """A decoder's window code as a header the referee's table knows: a decimated header whose second nybble is 0 or 1 (no row of
    FormatSpecs.md's table) is decoded by the reference as one full-size block, un-scaled (0) or scaled (1)."""
    wc = int(wc)
    if wc & 8 and (wc >> 4) < 2:
        return (wc & 7) if (wc >> 4) == 1 else 0
    return wc


# ---------------------------------------------------------------------------------------------------------------------
# arbitrary planes: the float64 referee
# ---------------------------------------------------------------------------------------------------------------------
def dec_code(h):
    """A header of ALL_CODES as the decoder forms WindowCtrl: | 0x10 behind a first nybble without bit 3."""
    return int(h) if h & 8 else int(h) | 0x10


@functools.lru_cache(maxsize=None)
def referee_case(bs, ch, seed):
    """Seeded normal coefficients under a seeded sequence of every header code (one plain block in front, three all-zero blocks in
    the middle) -> dict(coef [C][K][bs] float32, wc [K] decoder codes, ms [C][K * bs] and lr [C][K * bs]: the referee's PCM with and
    without the un-mix, float64, mid: the first all-zero block)."""
    headers = all_codes_sequence(seed, lead=[0])
    mid = len(headers) // 2
    headers[mid:mid] = [0, 0, 0]
    K = len(headers)
    rng = np.random.default_rng(seed)
    coef = rng.standard_normal((K, ch, bs)).astype(np.float32)
    coef[mid:mid + 3] = 0
    y = R.synthesise(coef.reshape(K, ch * bs), headers, bs, ch)[:K * bs]                    # [K bs][C], un-mixed
    return dict(coef=np.ascontiguousarray(coef.transpose(1, 0, 2)), wc=np.array([dec_code(h) for h in headers], np.int32),
                ms=np.ascontiguousarray(y.T), lr=np.ascontiguousarray(R.ms_fold(y).T), mid=mid, K=K)


def windows(K, n_out):
    """Output starts of WARM rows that together cover blocks 1 .. K - 1."""
    return list(range(1, K, n_out))


def case_rows(case, n_out, warm, key):
    """Rows over a referee case -> (coef [n][C][nPl][bs], wc [n][nPl], want [n][C][n_out * bs] float64, live [n][n_out])."""
    C, K, bs = case["coef"].shape
    firsts = windows(K, n_out) if warm else [0]
    n_pl = n_out + warm
    coef, wc = np.zeros((len(firsts), C, n_pl, bs), np.float32), np.zeros((len(firsts), n_pl), np.int32)
    want, live = np.zeros((len(firsts), C, n_out * bs)), np.zeros((len(firsts), n_out), np.int32)
    for i, first in enumerate(firsts):
        p0 = first - warm
        m, mo = min(n_pl, K - p0), min(n_out, K - first)
        coef[i, :, :m], wc[i, :m] = case["coef"][:, p0:p0 + m], case["wc"][p0:p0 + m]
        want[i, :, :mo * bs] = case[key][:, first * bs:(first + mo) * bs]
        live[i, :mo] = 1
    return coef, wc, want, live


def unit_rows(pcm, bs):
    """[n][C][nB * bs] -> [n][C][nB][bs]: one row per (row, channel, block) unit for R.unit_errors."""
    return pcm.reshape(pcm.shape[0], pcm.shape[1], -1, bs)
