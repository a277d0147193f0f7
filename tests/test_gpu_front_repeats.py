"""The encode call's front half where it no longer repeats work: k_wc_ef's producers load and M/S-convert
a sample once and take the neighbours' from the lanes beside them; k_cplx, not the transform, counts the non-zero
coefficients.  Every case against the oracle on the same input - sizes, WindowCtrl, BlockComplexity bit patterns,
coefficients and bytes (the comparison of tests/test_gpu_parity.py) - at the smallest shapes that reach the new edges."""
import numpy as np
import pytest

from gpu_testlib import amd as _amd
from ulc_testlib import synth_pcm, oracle_encode_debug
from test_gpu_parity import _compare_encode

pytestmark = pytest.mark.gpu

def _encode_calls(pcm, bs, rate, K, calls, mode=0, p0=50.0, taps=True, what=""):
    """`calls` consecutive calls of K blocks on one encoder, every stream and block against the oracle."""
    amd = _amd()
    B = pcm.shape[0]
    enc = amd.BatchEncoder(B, 2, bs, rate, K)
    refs = [oracle_encode_debug(pcm[s], bs, rate, mode, p0, slot=enc.slot) for s in range(B)]
    for j in range(calls):
        res = enc.encode(pcm[:, j * K * bs:(j + 1) * K * bs], mode, p0)
        dbg = enc.debug_fetch() if taps else None
        for s in range(B):
            _compare_encode(res, refs[s], s, j * K, K, dbg, what)
    enc.close()
    return refs


# ---------------------------------------------------------------------------
# A. k_wc_ef: one load and one M/S per sample, neighbours by lane exchange
# ---------------------------------------------------------------------------
def _impulse_pcm(B, n, bs, K, rate, seed):
    """Quiet tones with single-sample impulses (both M and S non-zero) at samples that are lane 0, lane 63 and the lanes
    beside a 16-lane row boundary of an envelope tile (a tile's lane = centre sample mod 64: BlockSize / 2 is a multiple
    of 64), in the first call's history-path tiles, at the border to its first fast tile, and in the second call."""
    pcm = np.stack([synth_pcm(s, n, 2, rate, transient=False, seed=seed) for s in range(B)]) * np.float32(0.05)
    call2 = K * bs
    spots = {0: [0, 64, bs // 2 + 64, call2 + 64 * 3, call2 + bs + 128],                    # lane 0 (the sample right of a tile)
             1: [63, bs // 2 + 63, call2 + 63, call2 + 64 * 5 + 63, call2 + bs + 127],      # lane 63 (the sample left of a tile)
             2: [15, 16, call2 + 64 * 2 + 15, call2 + 64 * 4 + 16, call2 + 64 * 6 + 31, call2 + 64 * 7 + 32, call2 + 64 * 9 + 47, call2 + 64 * 9 + 48]}
    for s in range(B):
        for t in spots[s % 3]:
            t += 64 * (s // 3)
            if t < n:
                pcm[s, t, 0] += np.float32(0.9 if s % 2 == 0 else -0.7)
                pcm[s, t, 1] -= np.float32(0.5)
    return pcm


# (BlockSize, B, K): (switched blocks over all streams, their WindowCtrl codes) of _impulse_pcm under the oracle
IMPULSE_CODES = {
    (256, 3, 2): (3, [0x49]), (256, 3, 3): (3, [0x49]), (256, 3, 5): (3, [0x49]),
    (256, 9, 2): (12, [0x49]), (256, 9, 3): (12, [0x49]), (256, 9, 5): (15, [0x49, 0x59, 0x69]),
    (2048, 3, 2): (6, [0x8B, 0xC9, 0xCA, 0xCB]), (2048, 3, 3): (8, [0x89, 0x8B, 0xC9, 0xCA, 0xCB]), (2048, 3, 5): (8, [0x89, 0x8B, 0xC9, 0xCB]),
    (2048, 9, 2): (18, [0x8B, 0xC9, 0xCA, 0xCB, 0xD9, 0xDB]), (2048, 9, 3): (21, [0x89, 0x8B, 0xC9, 0xCA, 0xCB, 0xDA, 0xDB]),
    (2048, 9, 5): (22, [0x89, 0x8B, 0xC9, 0xCB, 0xD9]),
}


@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("B", [3, 9])
@pytest.mark.parametrize("bs", [256, 2048])
def test_envelope_lane_exchange_matches_the_oracle(bs, B, K):
    """Stereo, a partial group of 8 streams (B = 3) and a second workgroup holding one stream (B = 9); K * BS / 64 tiles is
    and is not a multiple of the tiles in flight; two consecutive calls, so that the second call's history path reads real
    history; impulses at the tile edges, where a lane's neighbour is the other tile's sample."""
    rate = 44100
    pcm = _impulse_pcm(B, 2 * K * bs, bs, K, rate, seed=77 + K)
    refs = _encode_calls(pcm, bs, rate, K, 2, taps=False, what=f"wc_ef bs={bs} B={B} K={K}")
    switched = [int(c) for r in refs for c in r["wc"] if c != 0x10]
    assert (len(switched), sorted(set(switched))) == IMPULSE_CODES[bs, B, K], "the windows the impulses switch (the oracle's, which the calls above were held against)"


# ---------------------------------------------------------------------------
# B. the non-zero count comes from k_cplx
# ---------------------------------------------------------------------------
def _sparse_streams(bs, nblk):
    """0: all zero; 1: one non-zero sample; 2, 3: ordinary streams."""
    n = nblk * bs
    z = np.zeros((n, 2), np.float32)
    one = z.copy()
    one[bs + bs // 3, 0] = np.float32(0.25)
    return np.stack([z, one, synth_pcm(2, n, 2, 44100, transient=True, seed=9), synth_pcm(3, n, 2, 44100, transient=False, seed=9)])


@pytest.mark.parametrize("mode,p0", [(0, 50.0), (1, 64.0)])
def test_nonzero_count_of_empty_and_nearly_empty_streams(mode, p0):
    """An all-zero stream keeps nothing (MaxCoef = 0: nOutCoef 0, the bytes the oracle writes for an empty block); a stream
    with one non-zero sample has a few non-zero blocks among empty ones.  VBR (nOutCoef capped by the count) and CBR (the
    count bounds the search)."""
    bs, K = 2048, 4
    pcm = _sparse_streams(bs, 2 * K)
    amd = _amd()
    enc = amd.BatchEncoder(4, 2, bs, 44100, K)
    refs = [oracle_encode_debug(pcm[s], bs, 44100, mode, p0, slot=enc.slot) for s in range(4)]
    for j in range(2):
        res = enc.encode(pcm[:, j * K * bs:(j + 1) * K * bs], mode, p0)
        dbg = enc.debug_fetch()
        assert (dbg["nout"][0] == 0).all() and (dbg["coef"][0] == 0).all(), "the all-zero stream"
        for s in range(4):
            _compare_encode(res, refs[s], s, j * K, K, dbg if mode == 0 else None, f"sparse mode={mode}")
    assert (refs[0]["nout"] == 0).all()
    enc.close()


def test_nonzero_count_bounds_the_searches_of_a_two_rung_ladder():
    """VBR then CBR on four streams in one ladder call: the count k_cplx leaves is what arms the second rung's searches
    (k_rung_arm).  Each rung against an oracle encoder of its own: sizes, bytes; WindowCtrl and BlockComplexity once."""
    bs, K = 2048, 4
    pcm = _sparse_streams(bs, K)
    amd = _amd()
    enc = amd.BatchEncoder(4, 2, bs, 44100, K)
    rungs = [(0, 50.0, 0.0), (1, 64.0, 0.0)]
    out, bits, wc, cplx = enc.encode_ladder(pcm, rungs)
    for r, (mode, p0, p1) in enumerate(rungs):
        for s in range(4):
            ref = oracle_encode_debug(pcm[s], bs, 44100, mode, p0, p1, slot=enc.slot)
            _compare_encode((out[r], bits[r], wc, cplx), ref, s, 0, K, None, f"ladder rung {r}")
    enc.close()
