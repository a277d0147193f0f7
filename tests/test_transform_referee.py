"""The oracle's transform path, end to end, against the float64 referee written from FormatSpecs.md alone
(tests/mdct_referee.py): the encoder's sub-block walk and lapping FIFO up to its coefficients, the decoder's synthesis and
overlap-add down to its PCM, M/S and the 2/S normalisation, at every BlockSize and header code.  The HIP kernels are
bit-exact with the oracle (tests/test_gpu_parity.py) and are checked against the same referee on the GPU
(tests/test_gpu_transform_referee.py).

Tolerance: BASELINE.json north_star, 1e-5 of the peak |reference| per (block, channel); a unit whose reference is all zero
must come out as exact zeros.  Worst relative errors measured here (oracle encoder coefficients / oracle decoder PCM):
    BlockSize    256      512      1024     2048     4096     8192     16384    32768
    encoder      2.1e-07  2.2e-07  1.9e-07  1.8e-07  1.8e-07  1.7e-07  1.7e-07  1.4e-07
    decoder      3.0e-07  2.5e-07  2.4e-07  2.4e-07  2.5e-07  2.8e-07  2.5e-07  2.9e-07
"""
import numpy as np
import pytest
import mdct_referee as R
from ulc_testlib import oracle_encode_debug, oracle_decode_stream, oracle_decode_stream_coefs, spec_stream, synth_pcm

TOL = 1e-5
SIZES = (256, 512, 1024, 2048, 4096, 8192, 16384, 32768)
# every header code: overlap scale 0-7 x (no decimation, the 14 decimation patterns FormatSpecs.md allocates, 2h-Fh)
ALL_CODES = [s for s in range(8)] + [(p << 4) | 8 | s for p in range(2, 16) for s in range(8)]


def all_codes_sequence(seed, lead=()):
    rng = np.random.default_rng(seed)
    return list(lead) + [int(c) for c in rng.permutation(ALL_CODES)]


def transitions(wcs, N):
    """(nominal overlap, clipped overlap, previous sub-block size) of every transition after the stream's first."""
    out = []
    prev = None
    for wc in wcs:
        sizes, ovs = R.geometry(wc, N)
        for S, ov in zip(sizes, ovs):
            if prev is not None:
                out.append((ov, min(ov, prev), prev))
            prev = S
    return out


def transient_pcm(N, K, C, seed):
    """Tones + noise with dense decaying bursts (0.4-1.6 blocks apart, onsets over 2.3 decades), on the PCM16 grid."""
    rng = np.random.default_rng(seed)
    n = K * N
    x = synth_pcm(seed, n, C, 44100, transient=False, seed=seed).astype(np.float64) * 0.3
    pos = 0
    while True:
        pos += int(rng.uniform(0.4, 1.6) * N)
        if pos >= n:
            break
        ln = min(n - pos, int(rng.uniform(0.05, 1.0) * N) + 16)
        amp = 10 ** rng.uniform(-2.5, -0.2)
        x[pos:pos + ln] += rng.normal(0, amp, (ln, C)) * np.exp(-np.arange(ln) / (ln / 4))[:, None]
    return (np.clip(np.rint(x * 32768), -32768, 32767) / 32768).astype(np.float32)


# ---- the referee on its own ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [32, 64, 128, 256, 512, 1024, 2048])
def test_referee_fft_path_equals_direct_sum(S):
    rng = np.random.default_rng(S)
    f = rng.normal(size=(3, 2 * S))
    X = rng.normal(size=(3, S))
    for a, b in ((R.mdct(f, "direct"), R.mdct(f, "fft")), (R.imdct(X, "direct"), R.imdct(X, "fft"))):
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max()


@pytest.mark.parametrize("N,C", [(256, 3), (512, 2), (1024, 1), (4096, 6), (32768, 2)])
def test_referee_reconstructs_through_every_header_code(N, C):
    """analyse -> synthesise is the input delayed by 2 N, within 1e-12, over a random header sequence holding every header
    code; at the BlockSizes where they exist, overlaps 0 and 1 between sub-blocks and overlaps clipped to the previous
    sub-block are on the way."""
    wc = all_codes_sequence(N + C, lead=[0])
    tr = transitions(wc, N)
    if N <= 1024:
        assert any(ov == 1 for _, ov, _ in tr), "no one-sample overlap"
    if N <= 512:
        assert any(ov == 0 for _, ov, _ in tr), "no zero overlap between sub-blocks"
    assert any(nom > prev for nom, _, prev in tr), "no overlap clipped to the previous sub-block"
    K = len(wc)
    x = np.random.default_rng(C).normal(0, 0.3, (K * N, C))
    X = R.analyse(x, wc, N, method="fft" if N > 1024 else "auto")
    y = R.synthesise(X, wc, N, C, method="fft" if N > 1024 else "auto")[:(K - 1) * N]
    want = np.zeros_like(y)
    want[2 * N:] = x[:(K - 3) * N]
    assert np.abs(y - want).max() <= 1e-12 * np.abs(x).max()


def test_referee_one_sample_overlap_is_a_butterfly():
    """ov = 1: both samples that straddle the transition get sin(pi/4) in both the rising and the falling window."""
    d = np.arange(-3, 3)
    s4 = np.sin(np.pi / 4)
    assert np.array_equal(R.rise(d, 1), [0, 0, s4, s4, 1, 1])
    assert np.array_equal(R.fall(d, 1), [1, 1, s4, s4, 0, 0])
    assert np.array_equal(R.rise(d, 0), [0, 0, 0, 1, 1, 1])
    r2 = R.rise(d, 2)
    assert r2[:2].tolist() == [0, 0] and r2[4:].tolist() == [1, 1] and np.allclose(r2[2:4], np.sin(np.pi / 8 * np.array([1, 3])))


def test_referee_header_table():
    """Spot checks of FormatSpecs.md:35-51, read independently of the codec's decimation-pattern words."""
    assert R.geometry(0x05, 2048) == ([2048], [64])
    assert R.geometry(0x3B, 2048) == ([1024, 1024], [1024, 128])
    assert R.geometry(0x6F, 512) == ([256, 128, 128], [256, 1, 128])
    assert R.geometry(0xAE, 256) == ([64, 32, 32, 128], [64, 0, 32, 128])
    assert R.geometry(0xF9, 4096) == ([2048, 1024, 512, 512], [2048, 1024, 512, 256])
    with pytest.raises(ValueError):
        R.geometry(0x18, 2048)


# ---- the oracle's encoder ---------------------------------------------------------------------------------------------
# decimation patterns (second header nybble) the encoder chose for transient_pcm below, over all channel counts and both
# modes: what this test has covered, on record
ENC_PATTERNS = {256: {4, 5, 7}, 512: {8, 11, 13}, 1024: {8, 11, 12, 13, 15}, **{N: set(range(8, 16)) for N in SIZES[3:]}}


@pytest.mark.parametrize("N", SIZES)
def test_oracle_encoder_coefficients_match_referee(N):
    """oracle_encode_debug's coefficient tap (BlockTransform.c's TransformBuffer after the 2/S normalisation) against the
    referee's analysis of the same PCM and the headers the encoder wrote: 1, 2, 3 and 6 channels, VBR and CBR, on
    transient-heavy input; every block whose successor's header is known."""
    K = 24 if N <= 4096 else 10
    pats, worst = set(), 0.0
    for C in (1, 2, 3, 6):
        pcm = transient_pcm(N, K, C, seed=N + C)
        for mode, p0 in ((0, 50.0), (1, 96.0)):
            r = oracle_encode_debug(pcm, N, 44100, mode, p0)
            X = R.analyse(pcm, r["wc"], N)
            e = R.unit_errors(r["coef"][:-1].reshape(-1, C, N), X.reshape(-1, C, N))
            assert e.max() <= TOL, (C, mode, np.unravel_index(e.argmax(), e.shape), e.max())
            worst = max(worst, e.max())
            pats |= {int(w) >> 4 & 15 for w in r["wc"] if w & 8}
    assert pats >= ENC_PATTERNS[N], sorted(pats)
    print(f"N={N}: worst {worst:.2e}, patterns {sorted(pats)}")


# ---- the oracle's decoder ---------------------------------------------------------------------------------------------
DEC_CHANNELS = {256: 6, 512: 3, 1024: 2, 2048: 1, 4096: 6, 8192: 3, 16384: 2, 32768: 1}


def decoder_case(N, C, seed):
    """Every header code in a shuffled order behind two plain blocks, three silent blocks in the middle."""
    wc = all_codes_sequence(seed, lead=[0, 0x3])
    mid = len(wc) // 2
    wc[mid:mid] = [0x0, 0x0, 0x0]
    blocks, coefs, _ = spec_stream(wc, C, N, seed, silent_blocks=(mid, mid + 1, mid + 2))
    return wc, blocks, coefs, mid


@pytest.mark.parametrize("N", SIZES)
def test_oracle_decoder_pcm_matches_referee(N):
    """oracle_decode_stream's PCM against the referee's synthesis of the stream's coefficients (known exactly: the
    assembler wrote them, and oracle_decode_stream_coefs hands back the same), on a hand-assembled stream holding every
    header code; output blocks of a silent stretch are exact zeros."""
    C = DEC_CHANNELS[N]
    wc, blocks, coefs, mid = decoder_case(N, C, seed=N)
    assert {w if w & 8 else w & 7 for w in wc} >= set(ALL_CODES)
    rc, pcm, _, ocoefs = oracle_decode_stream_coefs(blocks, C, N)
    assert rc == 0
    assert np.array_equal(ocoefs, coefs)
    rc2, pcm2, _ = oracle_decode_stream(blocks, C, N)
    assert rc2 == 0 and np.array_equal(pcm2, pcm)
    K = len(wc)
    y = R.synthesise(coefs, wc, N, C)[:K * N]
    e = R.unit_errors(R.pcm_units(pcm, N), R.pcm_units(y, N))
    assert e.max() <= TOL, (np.unravel_index(e.argmax(), e.shape), e.max())
    assert not pcm[(mid + 1) * N:(mid + 3) * N].any() and not y[(mid + 1) * N:(mid + 3) * N].any()
    print(f"N={N} C={C}: worst {e.max():.2e}")


# ---- sensitivity: wrong readings of the spec must miss by far more than the tolerance ----------------------------------
@pytest.mark.parametrize("wrong", [dict(clip=False), dict(reverse=True), dict(shift=1), dict(plain_ov1=True)],
                         ids=["no_clip", "reversed", "shift1", "plain_ov1"])
@pytest.mark.parametrize("N", [256, 1024])
def test_wrong_referee_readings_miss(N, wrong):
    C = DEC_CHANNELS[N]
    wc, blocks, coefs, _ = decoder_case(N, C, seed=N)
    rc, pcm, _ = oracle_decode_stream(blocks, C, N)
    assert rc == 0
    K = len(wc)
    right = R.unit_errors(R.pcm_units(pcm, N), R.pcm_units(R.synthesise(coefs, wc, N, C)[:K * N], N))
    bad = R.unit_errors(R.pcm_units(pcm, N), R.pcm_units(R.synthesise(coefs, wc, N, C, **wrong)[:K * N], N))
    assert right.max() <= TOL
    assert bad.max() >= 100 * TOL, (wrong, bad.max())
