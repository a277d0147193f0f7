"""Pins the oracle's restatement of the three reference sources that compile on
their own (WindowControl, Psyopt, NoiseFill) to the REAL reference objects in
oracle/_ref/libulc_ref_partial.so — bit-exact, same inputs, same state threading.
Skipped only when build() left no oracle/_ref (no reference tree to compile it from)."""
import ctypes as C
import numpy as np
import pytest
from ulc_testlib import oracle, ref_partial, synth_pcm, ptr, f32p, i32p

REF = ref_partial()
needs_ref = pytest.mark.skipif(REF is None, reason="oracle/_ref not built: build() found no reference tree to compile it from")


def _chan_major_ms(pcm, bs, k):
    """[Old|New] SampleBuffer image for call k, after the encoder's M/S step."""
    n, ch = pcm.shape
    def blk(i):
        if i < 0:
            return np.zeros((ch, bs), np.float32)
        b = pcm[i * bs:(i + 1) * bs].T.copy()
        for c in range(1, ch, 2):
            l, r = b[c - 1].copy(), b[c].copy()
            b[c - 1] = (l + r) * np.float32(0.5)
            b[c] = (l - r) * np.float32(0.5)
        return b
    return np.ascontiguousarray(np.concatenate([blk(k - 1).reshape(-1), blk(k).reshape(-1)]))


@needs_ref
@pytest.mark.parametrize("bs,ch,rate,transient", [(2048, 2, 44100, True), (2048, 1, 44100, True), (4096, 2, 48000, True),
                                                 (256, 1, 44100, True), (512, 2, 32000, True), (2048, 2, 44100, False)])
def test_window_ctrl_matches_reference(bs, ch, rate, transient):
    lib = oracle()
    nblk = 48
    pcm = synth_pcm(3, nblk * bs, ch, rate, transient=transient, seed=bs)
    tb_o = np.zeros(32, np.float32); tf_o = np.zeros(3, np.float32)
    tb_r = np.zeros(32, np.float32); tf_r = np.zeros(3, np.float32)
    tmp_o = np.zeros(2 * bs, np.float32); tmp_r = np.zeros(2 * bs, np.float32)
    seen = set()
    for k in range(nblk):
        sb = _chan_major_ms(pcm, bs, k)
        wo = lib.orc_get_window_ctrl(ptr(sb, f32p), ptr(tb_o, f32p), ptr(tf_o, f32p), ptr(tmp_o, f32p), bs, ch, rate)
        wr = REF.ULCi_GetWindowCtrl(ptr(sb, f32p), ptr(tb_r, f32p), ptr(tf_r, f32p), ptr(tmp_r, f32p), bs, ch, rate)
        assert wo == wr, f"block {k}: oracle {wo:#x} reference {wr:#x}"
        assert tb_o.tobytes() == tb_r.tobytes()
        assert tf_o.tobytes() == tf_r.tobytes()
        seen.add(wr)
    if transient:
        assert len(seen) > 1, "transient signal should force some window switching"


@needs_ref
@pytest.mark.parametrize("bs,rate", [(2048, 44100), (4096, 48000), (256, 44100), (1024, 32000)])
def test_psychoacoustics_matches_reference(bs, rate):
    lib = oracle()
    rng = np.random.default_rng(bs)
    for wc in [0x10, 0x8B, 0x99, 0xAA, 0xBB, 0xC9, 0xDA, 0xEB, 0xF9, 0x2A, 0x3B, 0x49, 0x5A, 0x6B, 0x79]:
        amp = (rng.normal(0, 1, bs // 2) ** 2 * 10 ** rng.uniform(-12, 0, bs // 2)).astype(np.float32)
        amp[rng.integers(0, bs // 2, 8)] = 0.0
        if wc == 0x99:
            amp[: bs // 4] = 0.0   # silent bands carry the previous ratio
        a_o, a_r = amp.copy(), amp.copy()
        m_o = np.zeros(bs // 2, np.float32); m_r = np.zeros(bs // 2, np.float32)
        t_o = np.zeros(64, np.float32); t_r = np.zeros(64, np.float32)
        lib.orc_calc_psychoacoustics(ptr(m_o, f32p), ptr(a_o, f32p), t_o.ctypes.data, bs, rate, wc)
        REF.ULCi_CalculatePsychoacoustics(ptr(m_r, f32p), ptr(a_r, f32p), t_r.ctypes.data, bs, rate, wc)
        assert m_o.tobytes() == m_r.tobytes(), f"wc {wc:#x}"


@needs_ref
@pytest.mark.parametrize("n,rate", [(2048, 44100), (1024, 44100), (512, 48000), (256, 44100), (4096, 48000), (32, 44100)])
def test_noise_log_spectrum_matches_reference(n, rate):
    lib = oracle()
    rng = np.random.default_rng(n + rate)
    for trial in range(6):
        d = np.zeros(n, np.float32)
        d[: n // 2] = (rng.normal(0, 1, n // 2) ** 2 * 10 ** rng.uniform(-14, 0, n // 2)).astype(np.float32)
        if trial == 1:
            d[: n // 4] = 0
        if trial == 2:
            d[:] = 0
        d_o, d_r = d.copy(), d.copy()
        t_o = np.zeros(n + 64, np.float32); t_r = np.zeros(n + 64, np.float32)
        lib.orc_calc_noise_log_spectrum(ptr(d_o, f32p), t_o.ctypes.data, n, rate)
        REF.ULCi_CalculateNoiseLogSpectrum(ptr(d_r, f32p), t_r.ctypes.data, n, rate)
        assert d_o.tobytes() == d_r.tobytes()


@needs_ref
def test_noise_fill_params_match_reference():
    lib = oracle()
    rng = np.random.default_rng(7)
    n = 2048
    d = np.zeros(n, np.float32)
    d[: n // 2] = (rng.normal(0, 1, n // 2) ** 2 * 10 ** rng.uniform(-9, -2, n // 2)).astype(np.float32)
    # realistic {w, w*log} pairs come from the spectrum routine itself
    t = np.zeros(n, np.float32)
    REF.ULCi_CalculateNoiseLogSpectrum(ptr(d, f32p), t.ctypes.data, n, 44100)
    nq = 0
    for trial in range(400):
        band = int(rng.integers(0, n - 16)); cnt = int(rng.integers(16, min(527, n - band) + 1))
        q = float(2.0 ** rng.integers(5, 20))
        a = lib.orc_get_noise_q(ptr(d, f32p), band, cnt, q)
        b = REF.ULCi_GetNoiseQ(ptr(d, f32p), band, cnt, q)
        assert a == b
        nq += b != 0
        o1, o2 = np.zeros(1, np.int32), np.zeros(1, np.int32)
        r1, r2 = np.zeros(1, np.int32), np.zeros(1, np.int32)
        lib.orc_get_hfext_params(ptr(d, f32p), band, n - band, q, ptr(o1, i32p), ptr(o2, i32p))
        REF.ULCi_GetHFExtParams(ptr(d, f32p), band, n - band, q, ptr(r1, i32p), ptr(r2, i32p))
        assert (o1[0], o2[0]) == (r1[0], r2[0])
    assert nq > 20
    z = np.zeros(64, np.float32)
    assert lib.orc_get_noise_q(ptr(z, f32p), 0, 32, 1024.0) == REF.ULCi_GetNoiseQ(ptr(z, f32p), 0, 32, 1024.0) == 0


@needs_ref
def test_helper_header_matches_reference_directly():
    """ulcHelper.h:24-136 through oracle/ref_helper_harness.c (the reference's own header compiled in place):
    FastLog, the companded quantisers, the decimation pattern table and the Bark/line maps, bit for bit."""
    from golden.make_golden import helper_inputs
    lib = oracle()
    if not hasattr(REF, "ref_FastLog"):
        pytest.skip("prebuilt oracle/_ref predates the helper harness")
    f32 = lambda v: np.float32(v).tobytes()
    xs = helper_inputs()
    rng = np.random.default_rng(99)
    xs = np.concatenate([xs, (rng.uniform(-60, 60, 20000)).astype(np.float32), (2.0 ** rng.uniform(-40, 8, 20000)).astype(np.float32)])
    for v in xs:
        v = float(v)
        assert f32(lib.orc_fastlog(v)) == f32(REF.ref_FastLog(v)), v
        assert lib.orc_companded_quantize_unsigned(abs(v)) == REF.ref_CompandedQuantizeUnsigned(abs(v)), v
        assert lib.orc_companded_quantize(v) == REF.ref_CompandedQuantize(v), v
        for lim in (7, 8, 16):
            assert lib.orc_quant_coef_unsigned(abs(v), lim) == REF.ref_CompandedQuantizeCoefficientUnsigned(abs(v), lim)
            assert lib.orc_quant_coef(v, lim) == REF.ref_CompandedQuantizeCoefficient(v, lim)
    for w in range(16):
        assert lib.orc_decimation_pattern(w << 4) == REF.ref_SubBlockDecimationPattern(w << 4)
        assert lib.orc_decimation_pattern((w << 4) | 0xB) == REF.ref_SubBlockDecimationPattern((w << 4) | 0xB)
    for n, rate in ((1024, 44100), (128, 48000), (4096, 96000), (16, 8000)):
        nyq = float(np.float32(rate) * np.float32(0.5))
        for line in range(n):
            fo, fr = lib.orc_line_to_freq(line, nyq, n), REF.ref_LineToFreq(line, nyq, n)
            assert f32(fo) == f32(fr)
            assert f32(lib.orc_freq_to_bark(fo)) == f32(REF.ref_FreqToBark(fr))
    for b in np.arange(-1.0, 27.0, 0.125, dtype=np.float32):
        fo, fr = lib.orc_bark_to_freq(float(b)), REF.ref_BarkToFreq(float(b))
        assert f32(fo) == f32(fr)
        assert f32(lib.orc_freq_to_line(fo, 22050.0, 1024)) == f32(REF.ref_FreqToLine(fr, 22050.0, 1024))
