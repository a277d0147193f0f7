"""The sample-rate axis: what tests/test_band_plan_capi.py (CPU) and tests/test_gpu_rate_axis.py share.

RateHz decides at create time which Bark kernels an encoder runs ("Ring classes"): the band edges follow from
(BlockSize, RateHz), and the most bands the full-size tables have open at one line puts the object in one of three classes -
ring 0 (more than 8 open: k_nbark / k_pbark, lane per sub-block, for every block), ring 4 or ring 8 (k_bark_uniform /
k_bark_levels with that many snapshots per lane).  Every case below names the class it is there for as (ring, most): most is
None where the class is the ring alone, a number where the count itself is the point - 9 is ring 0 just over the limit, 7 the
deepest ring 8 that is not full, most == ring a ring exactly full (a snapshot slot is reused by the next band at once).  The
CPU test asserts from ulcx_debug_band_plan that every case is in its class on this libm; the GPU test asserts the ring again
from the object it opened (ulcx_encoder_debug_plan).  All named rates are in their class here as they stand: none was moved.
"""
import numpy as np
from ulc_testlib import synth_pcm, oracle_encode_debug

MODE_VBR, MODE_CBR, MODE_ABR = 0, 1, 2
VBR50 = (MODE_VBR, 50.0, 0.0)
CBR64 = (MODE_CBR, 64.0, 0.0)
ABR96 = (MODE_ABR, 96.0, 0.45)

# (BlockSize, channels, RateHz, (ring, most))
BATCH_CASES = [
    # stereo 2048: steady-state k_xf, fused k_wc_ef, k_select_wave, direct packing
    (2048, 2, 8000, (0, None)), (2048, 2, 11025, (0, 9)), (2048, 2, 16000, (8, 7)), (2048, 2, 192000, (4, 4)),
    # stereo 4096: k_select_pair
    (4096, 2, 8000, (0, None)), (4096, 2, 16000, (8, None)), (4096, 2, 384000, (4, 4)),
    # mono 1024
    (1024, 1, 11025, (0, None)), (1024, 1, 22050, (8, None)), (1024, 1, 96000, (4, 4)),
    # 3 channels 512: the generic loop, an unpaired channel
    (512, 3, 8000, (0, None)), (512, 3, 192000, (8, 8)), (512, 3, 44100, (4, 4)),
    # stereo 256
    (256, 2, 96000, (8, 8)), (256, 2, 192000, (0, None)),
]
# further rate modes on top of VBR 50
MODE_CASES = [(2048, 2, 8000, (0, None), CBR64), (2048, 2, 16000, (8, 7), CBR64), (4096, 2, 8000, (0, None), CBR64),
              (1024, 1, 11025, (0, None), ABR96)]
# big blocks (k_xf_big above 8192); the 8192 pair: k_nsums at the largest block it takes / the exact path's heap in the object's scratch
# (BlockSize, channels, RateHz, (ring, most), plan fields the case is there for)
BIG_CASES = [
    (16384, 1, 16000, (8, None), {}), (16384, 1, 8000, (0, None), {}),
    (8192, 2, 16000, (8, None), dict(use_gap_sums=1, heap_in_lds=1)), (8192, 3, 8000, (0, None), dict(use_gap_sums=0, heap_in_lds=0)),
]
# whole tiles of decimated rows, and the two encoders of different rings on one device
TILE_CASES = [(2048, 2, 44100, (4, None)), (2048, 2, 16000, (8, 7))]
PAIR_CASES = [(2048, 2, 8000, (0, None)), (2048, 2, 44100, (4, None))]

ALL_CLASSED = sorted({(bs, rate, cls) for bs, _, rate, cls in BATCH_CASES + TILE_CASES + PAIR_CASES} |
                     {(c[0], c[2], c[3]) for c in MODE_CASES + BIG_CASES})


def in_class(most, ring, cls):
    want_ring, want_most = cls
    return ring == want_ring and (want_most is None or most == want_most)


def case_id(c):
    cls = c[3]
    return "%dx%d@%d-ring%d%s" % (c[0], c[1], c[2], cls[0], "" if cls[1] is None else "-open%d" % cls[1])


# ---------------------------------------------------------------------------
# the five distinct streams of a batch
# ---------------------------------------------------------------------------
def _grid16(x):
    return (np.clip(np.rint(x * 32768.0), -32768, 32767) * (1.0 / 32768.0)).astype(np.float32)


def white_noise(n, ch, seed):
    """Every Bark band of every block has energy."""
    return _grid16(np.random.default_rng([0xA71, seed]).normal(0.0, 0.1, (n, ch)))


def last_channel_silent(n, ch, rate, seed):
    """The last channel is digital silence: all its Bark bands are without energy, so every level of k_bark_levels is the
    carried-over one (mono: the whole stream)."""
    x = synth_pcm(7, n, ch, rate, transient=True, seed=seed).copy()
    x[:, ch - 1] = 0.0
    return x


def impulse_per_block(n, ch, bs, seed):
    """A burst of 48 samples (32 at BlockSize 256) three quarters into every block over a floor 55 dB below it.  Where a block
    lasts tens of milliseconds (BlockSize 2048 and up at 8 .. 48 kHz) window control decimates every block behind the stream's
    first; where it lasts a few, the detector's envelopes run the bursts together and only the first two or three blocks
    are decimated.  A test that depends on the window codes asserts them from the oracle's."""
    rng = np.random.default_rng([0x1A9, seed])
    x = rng.normal(0.0, 1e-3, (n, ch))
    for k in range(n // bs):
        p = k * bs + (3 * bs) // 4
        ln = min(bs // 8, 48)
        x[p:p + ln] += rng.normal(0.0, 0.6, (ln, ch)) * np.exp(-np.arange(ln) / 40.0)[:, None]
    return _grid16(x)


def distinct_streams(bs, ch, rate, nblk, seed):
    """[5][nblk * bs][ch]: two of synth_pcm with transients, white noise, last channel silent, an impulse in every block."""
    n = nblk * bs
    return np.stack([synth_pcm(0, n, ch, rate, transient=True, seed=seed), synth_pcm(1, n, ch, rate, transient=True, seed=seed + 1),
                     white_noise(n, ch, seed), last_channel_silent(n, ch, rate, seed), impulse_per_block(n, ch, bs, seed)])


IMPULSE = 4         # its row in distinct_streams


def tiled(distinct, B, seed):
    """B streams tiled from the distinct ones in a seeded permutation -> (pcm [B][n][ch], the distinct row of each stream)."""
    src = np.random.default_rng([0x71E, seed]).permutation(np.arange(B) % len(distinct))
    return distinct[src], src


def oracle_refs(distinct, bs, rate, mode, slot):
    return [oracle_encode_debug(d, bs, rate, mode[0], mode[1], mode[2], slot=slot) for d in distinct]


def decimated(wc):
    return (np.asarray(wc) & 8) != 0


# ---------------------------------------------------------------------------
# the comparison: sizes, WindowCtrl, BlockComplexity bit patterns and bytes; no tolerance anywhere
# ---------------------------------------------------------------------------
def compare_call(res, refs, src, k0, what):
    """One call's results (out [B][K][slot], bits, wc, cplx) against blocks [k0, k0 + K) of each stream's oracle encode."""
    out, bits, wc, cplx = res
    B, K = bits.shape
    sl = slice(k0, k0 + K)
    r_wc = np.stack([refs[i]["wc"][sl] for i in src])
    r_bits = np.stack([refs[i]["bits"][sl] for i in src])
    r_cplx = np.stack([refs[i]["cplx"][sl] for i in src])

    def first(bad):
        s, k = np.argwhere(bad)[0]
        return int(s), int(k), f"{what}: stream {s} (distinct {src[s]}) block {k0 + k}"

    bad = wc != r_wc
    if bad.any():
        s, k, tag = first(bad)
        raise AssertionError(f"{tag}: WindowCtrl {wc[s, k]:#x} != {r_wc[s, k]:#x} ({int(bad.sum())} blocks differ)")
    bad = np.ascontiguousarray(cplx).view(np.uint32) != np.ascontiguousarray(r_cplx).view(np.uint32)
    if bad.any():
        s, k, tag = first(bad)
        raise AssertionError(f"{tag}: BlockComplexity {cplx[s, k]!r} != {r_cplx[s, k]!r} ({int(bad.sum())} blocks differ)")
    bad = bits != r_bits
    if bad.any():
        s, k, tag = first(bad)
        raise AssertionError(f"{tag}: size {bits[s, k]} != {r_bits[s, k]} bits ({int(bad.sum())} blocks differ)")
    assert (bits > 0).all() and (bits % 8 == 0).all(), f"{what}: a block of no whole bytes (ulcEncoder_Encode.c:358 rounds every size up)"
    at = np.arange(out.shape[2])[None, :]
    for s in range(B):
        diff = (out[s] != refs[src[s]]["out"][sl]) & (at < (bits[s] // 8)[:, None])
        if diff.any():
            k, i = np.argwhere(diff)[0]
            raise AssertionError(f"{what}: stream {s} (distinct {src[s]}) block {k0 + k}: bytes differ from byte {i} of {bits[s, k] // 8}")
