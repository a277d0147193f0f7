"""The HIP transform path against the float64 referee written from FormatSpecs.md alone (tests/mdct_referee.py): the
encoder's coefficient tap (k_xf up to BlockSize 8192, k_xf_big at 16384 / 32768) against the referee's analysis, the
decoder's PCM (k_dsyn, whole streams, the even cut and the cut last round) against the referee's synthesis, and the
referee's synthesis of the GPU's own coefficients against the input delayed by 2 N.

Tolerance: BASELINE.json north_star, 1e-5 of the peak |reference| per (stream, block, channel); a unit whose reference is
all zero must come out as exact zeros.  The kernels are bit-exact with the oracle, so the worst errors are the oracle's
(tests/test_transform_referee.py); measured on an MI355X (encoder tap / decoder PCM):
    BlockSize    256      512      1024     2048     4096     8192     16384    32768
    encoder      1.7e-07  1.7e-07  1.6e-07  1.9e-07  1.5e-07  1.4e-07  1.3e-07  1.3e-07
    decoder      2.8e-07  2.4e-07  2.8e-07  2.8e-07  2.6e-07  3.0e-07  3.2e-07  2.7e-07
"""
import os
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
from gpu_testlib import amd as _amd
import mdct_referee as R
from ulc_testlib import spec_stream
from test_transform_referee import TOL, ALL_CODES, transient_pcm, decoder_case

pytestmark = pytest.mark.gpu


def _check_tap(pcm, wc, coef, N, C, what):
    """pcm [B][n][C], wc [B][K], coef [B][K][C*N]: every block whose successor's header is known -> worst error."""
    worst = 0.0
    for s in range(pcm.shape[0]):
        X = R.analyse(pcm[s], wc[s], N)
        e = R.unit_errors(coef[s, :-1].reshape(-1, C, N), X.reshape(-1, C, N))
        assert e.max() <= TOL, f"{what}: stream {s} (block, channel) {np.unravel_index(e.argmax(), e.shape)}: {e.max():.3e}"
        worst = max(worst, float(e.max()))
    return worst


# ---- encoder -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,calls", [
    (256, 6, (3, 1, 4)), (512, 1, (2, 3)), (1024, 3, (1, 4, 2)), (2048, 2, (3, 1, 4)),
    (4096, 6, (2, 2)), (8192, 1, (3, 1, 2)),                      # k_xf
    (16384, 2, (2, 1, 2)), (32768, 3, (2, 2)), (32768, 6, (1, 2)),  # k_xf_big
])
def test_encoder_tap_matches_referee_across_calls(N, C, calls):
    """Several calls of varying K on one encoder: each call's coefficient tap is kept, and a call's last block is checked
    once the next call has returned its successor's header."""
    amd = _amd()
    B, K = 3, sum(calls)
    pcm = np.stack([transient_pcm(N, K, C, seed=N + 10 * C + s) for s in range(B)])
    enc = amd.BatchEncoder(B, C, N, 44100, max(calls))
    wc, coef = [], []
    k0 = 0
    for k in calls:
        _, _, w, _ = enc.encode(pcm[:, k0 * N:(k0 + k) * N], amd.MODE_VBR, 50.0)
        coef.append(enc.debug_fetch(k, parts=("coef",))["coef"])
        wc.append(w)
        k0 += k
    enc.close()
    wc, coef = np.concatenate(wc, axis=1), np.concatenate(coef, axis=1)
    assert any(w & 8 for w in wc.ravel()), "no window switch on the way"
    worst = _check_tap(pcm, wc, coef, N, C, f"N={N} C={C}")
    print(f"encoder N={N} C={C}: worst {worst:.2e}")


def _benched_tap(cfg_name, B):
    """One call at a benched configuration's shape and input (bench.py's generator and seed for that configuration) ->
    (pcm [B][K N][2] host, wc [B][K], coefficient tap [B][K][2 N])."""
    import torch
    amd = _amd()
    sys.path.insert(0, ROOT)
    import bench
    cfg = bench.CONFIGS[cfg_name]
    K, N, rate = cfg["blocks"], cfg["bs"], cfg["rate"]
    dev = torch.device("cuda", 0)
    keep, bench.RATE = bench.RATE, rate
    try:
        pcm = bench.make_pcm(torch, B, K * N, dev, seed=4321, bursts_per_s=cfg["bursts"], decades=cfg["decades"])
    finally:
        bench.RATE = keep
    enc = amd.BatchEncoder(B, bench.CH, N, rate, K)
    out = torch.zeros(B, K, enc.slot, dtype=torch.uint8, device=dev)
    bits = torch.zeros(B, K, dtype=torch.int32, device=dev)
    wc = torch.zeros(B, K, dtype=torch.int32, device=dev)
    enc.encode_dev(pcm.data_ptr(), K, out.data_ptr(), bits.data_ptr(), wc.data_ptr(), 0,
                   mode=amd.MODE_VBR if cfg["mode"] == "vbr" else amd.MODE_CBR, p0=cfg["p0"])
    torch.cuda.synchronize()
    del out, bits
    coef = enc.debug_fetch(K, parts=("coef",))["coef"]
    enc.close()
    pcm_h, wc_h = pcm.cpu().numpy(), wc.cpu().numpy()
    del pcm
    torch.cuda.empty_cache()
    return pcm_h, wc_h, coef, N


def test_encoder_tap_at_wswitch_4096_benched_shape():
    """bench.py's wswitch_4096 step at one GPU's share (2048 stereo streams x 16 blocks of 4096, 1 GiB of coefficients):
    every block of every stream whose successor's header is known."""
    pcm, wc, coef, N = _benched_tap("wswitch_4096", 2048)
    assert coef.shape == (2048, 16, 2 * 4096)
    assert (wc & 8).any(axis=1).mean() > 0.5, "most streams should switch windows"
    for s0 in range(0, 2048, 256):
        _check_tap(pcm[s0:s0 + 256], wc[s0:s0 + 256], coef[s0:s0 + 256], N, 2, f"wswitch_4096 streams {s0}+")


def test_encoder_tap_at_headline_geometry_multi_round():
    """The headline geometry (vbr50: stereo BlockSize 2048, 32 blocks a call) at 320 streams: more workgroups than one
    round of the schedules; every stream."""
    pcm, wc, coef, N = _benched_tap("vbr50", 320)
    assert N == 2048 and coef.shape == (320, 32, 4096)
    _check_tap(pcm, wc, coef, N, 2, "vbr50 x 320")


def test_gpu_round_trip_through_referee_synthesis():
    """The referee's synthesis of the GPU's own coefficient tap is the input delayed by 2 N (the encoder's overlaps read
    with the decoder's convention, without the oracle).  Compared from the first output block that holds input on; the
    blocks before it hold only the float32 rounding of zero-input aliasing."""
    amd = _amd()
    for N, C, K in ((256, 3, 40), (2048, 2, 24), (16384, 1, 8), (32768, 2, 6)):
        B = 2
        pcm = np.stack([transient_pcm(N, K, C, seed=7 * N + s) for s in range(B)])
        enc = amd.BatchEncoder(B, C, N, 44100, K)
        _, _, wc, _ = enc.encode(pcm, amd.MODE_VBR, 50.0)
        coef = enc.debug_fetch(K, parts=("coef",))["coef"]
        enc.close()
        for s in range(B):
            y = R.synthesise(coef[s, :K - 1], wc[s], N, C)[:(K - 1) * N]
            want = np.zeros_like(y)
            want[2 * N:] = pcm[s, :(K - 3) * N]
            assert not y[:N].any()
            e = R.unit_errors(R.pcm_units(y[2 * N:], N), R.pcm_units(want[2 * N:], N))
            assert e.max() <= TOL, (N, C, s, np.unravel_index(e.argmax(), e.shape), e.max())


# ---- decoder -----------------------------------------------------------------------------------------------------------
def _decode(amd, blocks, C, N, calls):
    """blocks [B][K][slot] through one decoder in calls of the given sizes -> PCM [B][K N][C], or None at the documented
    LDS limit of the decoder."""
    try:
        dec = amd.BatchDecoder(blocks.shape[0], C, N, max(calls))
    except amd.UlcError as e:
        assert "LDS" in str(e) or "not built" in str(e), e
        return None, None
    out, k0 = [], 0
    for k in calls:
        p, bits = dec.decode(blocks[:, k0:k0 + k])
        assert (bits > 0).all()
        out.append(p)
        k0 += k
    cut = dec.last_cut()
    dec.close()
    return np.concatenate(out, axis=1), cut


@pytest.mark.parametrize("N,C", [(256, 6), (512, 3), (1024, 2), (2048, 1), (2048, 2), (4096, 6), (8192, 3), (16384, 2),
                                 (32768, 1), (32768, 2)])
def test_decoder_pcm_matches_referee_every_header_code(N, C):
    """Hand-assembled streams holding every header code (overlap scales 0-7, all 14 patterns, overlaps 1 and 0 where the
    BlockSize has them), three silent blocks in the middle, decoded in three calls."""
    amd = _amd()
    cases = [decoder_case(N, C, seed=N + 100 * C + s) for s in range(2)]
    K = len(cases[0][0])
    slot = max(c[1].shape[1] for c in cases)
    blocks = np.zeros((2, K, slot), np.uint8)
    for s, c in enumerate(cases):
        blocks[s, :, :c[1].shape[1]] = c[1]
    got, _ = _decode(amd, blocks, C, N, (40, 1, K - 41))
    if got is None:
        return
    worst = 0.0
    for s, (wc, _, coefs, mid) in enumerate(cases):
        assert {w if w & 8 else w & 7 for w in wc} >= set(ALL_CODES)
        y = R.synthesise(coefs, wc, N, C)[:K * N]
        e = R.unit_errors(R.pcm_units(got[s], N), R.pcm_units(y, N))
        assert e.max() <= TOL, (s, np.unravel_index(e.argmax(), e.shape), e.max())
        assert not got[s, (mid + 1) * N:(mid + 3) * N].any()
        worst = max(worst, float(e.max()))
    print(f"decoder N={N} C={C}: worst {worst:.2e}")


def _tiled_decode_check(amd, B, K, N, C, calls, n_distinct=8):
    """B streams tiled from n_distinct hand-assembled ones (random header codes), decoded in `calls`; every stream against
    the referee's synthesis of its pattern -> the decoder's last_cut()."""
    pats = []
    for i in range(n_distinct):
        wc = [0] + [int(c) for c in np.random.default_rng(50 + i).choice(ALL_CODES, K - 1)]
        blocks, coefs, _ = spec_stream(wc, C, N, 60 + i)
        pats.append((wc, blocks, coefs))
    slot = max(p[1].shape[1] for p in pats)
    blocks = np.zeros((B, K, slot), np.uint8)
    for s in range(B):
        b = pats[s % n_distinct][1]
        blocks[s, :, :b.shape[1]] = b
    got, cut = _decode(amd, blocks, C, N, calls)
    assert got is not None
    for i, (wc, _, coefs) in enumerate(pats):
        y = R.synthesise(coefs, wc, N, C)[:K * N]
        ref = R.pcm_units(y, N)
        for s in range(i, B, n_distinct):
            e = R.unit_errors(R.pcm_units(got[s], N), ref)
            assert e.max() <= TOL, (s, np.unravel_index(e.argmax(), e.shape), e.max())
    return cut


def test_decoder_even_cut_matches_referee():
    """Few long streams: ulcx_dec_split_plan cuts the synthesis evenly over the device (pieces start mid-stream)."""
    amd = _amd()
    B, K, N, C = 16, 64, 2048, 2
    grid, whole, resident = _tiled_decode_check(amd, B, K, N, C, (K,))
    assert resident > 0 and grid > 0 and whole == 0, (grid, whole, resident)
    assert grid == amd.lib().ulcx_dec_split_plan(B, K, resident)


def test_decoder_tail_cut_matches_referee():
    """Whole rounds plus a last round two thirds full, 26 blocks a call: ulcx_dec_tail_plan cuts the last round's streams
    into pieces; every stream checked, two calls."""
    import ctypes as Ct
    amd = _amd()
    N, C, K = 2048, 2, 26
    probe = amd.BatchDecoder(8, C, N, K)
    resident = probe.last_cut()[2]
    probe.close()
    assert resident > 0
    B = resident + resident * 2 // 3
    full = Ct.c_int32(0)
    tail = amd.lib().ulcx_dec_tail_plan(B, K, resident, Ct.byref(full))
    assert amd.lib().ulcx_dec_split_plan(B, K, resident) == 0 and tail > 0
    grid, whole, _ = _tiled_decode_check(amd, B, 2 * K, N, C, (K, K), n_distinct=16)
    assert whole == full.value and grid == full.value + tail, (grid, whole, full.value, tail)
