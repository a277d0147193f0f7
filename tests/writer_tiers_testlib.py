"""Inputs and predictions of the writer-tier tests (tests/test_writer_tiers_capi.py, tests/test_gpu_writer_tiers.py).

k_encode_wave writes every block through a ladder of capacity tiers (small -> medium or full -> the serial k_encode_units); a
unit leaves a tier for one of four reasons (encode_unit_wave, csrc/ulcx_enc_wr.hip):
  K  more kept coefficients than the tier holds          Z  more zones of the greedy max > 4*min segmentation
  N  more nybbles                                         G  the run codes of one gap exceed 32 nybbles (whatever the tier)
This file counts K, Z, N and G per (block, channel, sub-block) unit FROM THE ORACLE ALONE and predicts from them, and from the
capacities the library reports (ulcx_encoder_debug_writer_plan), the flags ulcx_encoder_debug_writer_flags must give per block.
The signal generators sit here too, so that the CPU test can check that each input has the property its GPU test is named for.
CPU only; nothing here runs the library under test."""
import functools
import numpy as np
from ulc_testlib import oracle_encode_debug
from spectra_testlib import subblocks_of
from spec_decoder import decode_block_coefficients

RATE = 44100
GAP_NYBBLES = 32                                            # cause G: the run codes of one gap, in no tier more than this


# ---------------------------------------------------------------------------------------------------------------------
# counts per unit, from the oracle's intermediates and bytes
# ---------------------------------------------------------------------------------------------------------------------
def zones_of(levels):
    """Zones the greedy rule of Encode.c:218-269 cuts a unit's kept levels (absolute values, in order) into, in binary32: the
    first coefficient's minimum is capped at 1000, a zone closes in front of the first coefficient that makes max > 4*min over
    the zone so far, a last zone whose maximum is zero is not counted."""
    lv = np.abs(np.asarray(levels, np.float32))
    if lv.size == 0:
        return 0
    four = np.float32(4.0)
    mn, mx, n = min(lv[0], np.float32(1000.0)), lv[0], 0
    for v in lv[1:]:
        nmn, nmx = min(mn, v), max(mx, v)
        if nmx > np.float32(nmn * four):
            n += 1
            mn = mx = v
        else:
            mn, mx = nmn, nmx
    return n + (1 if mx != 0 else 0)


def block_units(ref, k, ch, bs):
    """Units of block k of an oracle_encode_debug result, in coded order: dicts ch, j, size, off (inside the channel), nK (kept
    coefficients: rank < nout), nZ (zones_of the kept coefficients), nyb (the unit's nybbles in the block's bytes), changes
    (quantizer-change codes in them) and gap (the most run-code nybbles of one gap) - the last three from the walk of the
    bytes by tests/spec_decoder.py."""
    sizes = subblocks_of(bs, int(ref["wc"][k]))
    walk = []
    nbytes = int(ref["bits"][k]) // 8
    _, _, used = decode_block_coefficients(ref["out"][k, :nbytes], ch, bs, units=walk)
    assert (used + 1) // 2 == nbytes and len(walk) == ch * len(sizes), (used, nbytes, len(walk))
    keep = ref["ranks"][k] < ref["nout"][k]
    out = []
    for c in range(ch):
        off = 0
        for j, S in enumerate(sizes):
            w = walk[c * len(sizes) + j]
            assert (w["ch"], w["j"], w["size"]) == (c, j, S)
            lo = c * bs + off
            kept = keep[lo:lo + S]
            out.append(dict(ch=c, j=j, size=S, off=off, nK=int(kept.sum()), nZ=zones_of(ref["coef"][k, lo:lo + S][kept]), nyb=w["nyb"],
                            changes=w["quantizer_changes"], gap=w["max_gap_run_nybbles"]))
            off += S
    return out


def stream_units(ref, ch, bs):
    return [block_units(ref, k, ch, bs) for k in range(ref["nout"].shape[0])]


def whole(units, ch):
    """un-decimated block: one unit per channel"""
    return len(units) == ch


# ---------------------------------------------------------------------------------------------------------------------
# prediction
# ---------------------------------------------------------------------------------------------------------------------
def causes(u, caps):
    """The reasons unit u leaves a tier of capacities caps = (kept, zones, nybbles): a subset of "KZNG".  (The kernel tests them in
    this order and stops at the first; any one hands the block over.)"""
    return "".join(c for c, over in (("K", u["nK"] > caps[0]), ("Z", u["nZ"] > caps[1]), ("N", u["nyb"] > caps[2]), ("G", u["gap"] > GAP_NYBBLES)) if over)


def predict_flags(units, plan, ch, exact=False, direct=True):
    """Flags of one block from its units' counts and the reported plan.  exact: the block is on the exact (heapsort-rank) path,
    whose retry runs on the medium tier where the geometry has one.  direct: the block's launch makes one trip and
    ULCX_DIRECT_PACK is not 0 (the main path's launch always makes one trip; the exact path's while its blocks fit its grid)."""
    flags = 0
    if any(causes(u, plan["small"]) for u in units):
        if not plan["have_full"]:
            flags = 2                                                               # one launch: straight to k_encode_units
        else:
            retry = plan["medium"] if (exact and plan["have_mid"]) else plan["full"]
            flags = 1 | (2 if any(causes(u, retry) for u in units) else 0)
    if flags == 0 and ch == 2 and whole(units, ch) and direct:
        flags = 4
    return flags


def exact_trip_is_single(n_blocks_call, n_exact, ch):
    """The exact path's launches of k_encode_wave: min(blocks of the call, 128) workgroups of four waves over n_exact blocks
    of ch channels (one group of rank slots).  Direct packing needs every wave to make one trip."""
    return min(n_blocks_call, 128) * 4 >= n_exact * ch


# ---------------------------------------------------------------------------------------------------------------------
# signals.  All deterministic; PCM on the 16-bit grid as a WAV reader gives it, [n][ch] float32.
# ---------------------------------------------------------------------------------------------------------------------
def _grid(x):
    return (np.clip(np.rint(np.asarray(x, np.float64) * 32768.0), -32768, 32767) / 32768.0).astype(np.float32)


def _peak(x, peak):
    return x * (peak / np.max(np.abs(x)))


def noise_pcm(n, ch, seed, amp=0.25):
    """dense: white noise, independent per channel"""
    rng = np.random.default_rng([0x717E5, seed])
    return _grid(amp * rng.standard_normal((n, ch)))


def comb_pcm(n, bs, first, step, count, amps=(1.0,), peak=0.9, rate=RATE, seed=0):
    """`count` steady tones on the bin centres (k + 0.5) * rate / (2 * bs), k = first + step * i, amplitudes cycling through
    `amps`, random phases, scaled to `peak`.  Mono [n][1]."""
    rng = np.random.default_rng([0xC03B, seed])
    t = np.arange(n, dtype=np.float64) / rate
    x = np.zeros(n)
    for i in range(count):
        f = (first + step * i + 0.5) * rate / (2.0 * bs)
        x += amps[i % len(amps)] * np.sin(2 * np.pi * f * t + rng.uniform(0, 2 * np.pi))
    return _grid(_peak(x, peak))[:, None]


def z_comb(n, bs=2048):
    """Z alone: 150 tones four bins apart, alternating 1 and 1/32 - every tone its own zone"""
    return comb_pcm(n, bs, 60, 4, 150, (1.0, 1.0 / 32.0))


def n_comb(n, bs=2048):
    """N alone: 580 equal tones three bins apart - a run code between any two, three nybbles a kept coefficient, few zones.
    (440 tones four bins apart reach 1280 nybbles only with more than 460 kept coefficients, 90 % of that capacity.)"""
    return comb_pcm(n, bs, 40, 3, 580)


def sparse_pcm(n, rate, seed, floor, tones=3, fmax=2000.0, top=0.9):
    """G: a few low tones, one tone at `top` of the Nyquist frequency and nothing between them but a floor - the gap in front of
    the top tone's coefficients is thousands of zeros (what lies behind a unit's last kept coefficient is its end, not a gap)"""
    rng = np.random.default_rng([0x6A9, seed])
    t = np.arange(n, dtype=np.float64) / rate
    x = 0.25 * np.sin(2 * np.pi * (top * rate / 2) * t)
    for f, a in zip(rng.uniform(100.0, fmax, tones), rng.uniform(0.1, 0.3, tones)):
        x += a * np.sin(2 * np.pi * f * t + rng.uniform(0, 6.28))
    return _grid(x + floor * rng.standard_normal(n))[:, None]


def stereo_from_mid_side(mid, side):
    """[n] mid, [n] side -> [n][2] left = mid + side, right = mid - side (the coder codes (L+R)/2 and (L-R)/2)"""
    return _grid(np.stack([mid + side, mid - side], axis=1))


def burst_pcm(n, ch, bs, block, seed, bed=0.02, burst=0.9, at=0.8, length=None):
    """Decimated: a dense noise bed with one strong burst starting `at` of the way into block `block`."""
    rng = np.random.default_rng([0xB0257, seed])
    x = bed * rng.standard_normal((n, ch))
    p, ln = int((block + at) * bs), length or bs // 8
    x[p:p + ln] += burst * rng.standard_normal((ln, ch)) * np.exp(-np.arange(ln) / (ln / 4.0))[:, None]
    return _grid(np.clip(x, -0.99, 0.99))


# ---------------------------------------------------------------------------------------------------------------------
# solving a VBR quality for a kept count
# ---------------------------------------------------------------------------------------------------------------------
def quality_for_nout(pcm, bs, block, want, rate=RATE):
    """A float32 VBR quality at which the oracle keeps exactly `want` coefficients in block `block` of pcm.  In VBR
    nout = (int)(N * cplx / (0x1.E4EFB7p3f * logf(100 / q))) (ulcEncoder.c:144) and BlockComplexity does not depend on the
    quality, so nout grows with it: bisection on the oracle itself.  None if no float32 quality gives it."""
    def nout(q):
        return int(oracle_encode_debug(pcm, bs, rate, 0, float(q))["nout"][block])
    lo, hi = np.float32(1.0), np.float32(99.9999)
    if nout(lo) > want or nout(hi) < want:
        return None
    for _ in range(64):
        mid = np.float32((np.float64(lo) + np.float64(hi)) / 2)
        if mid == lo or mid == hi:
            break
        m = nout(mid)
        if m == want:
            return mid
        if m < want:
            lo = mid
        else:
            hi = mid
    for q in (lo, hi):
        if nout(q) == want:
            return q
    return None


def straddles(ref, k):
    """The threshold tie group of block k straddles the cut (more than nout keys are >= the nout-th largest): the selection
    hands such a block to the exact path by itself."""
    n = int(ref["nout"][k])
    keys = ref["keys"][k]
    if n <= 0 or n >= keys.size:
        return False
    T = np.partition(keys, keys.size - n)[keys.size - n]
    return int((keys >= T).sum()) > n


# ---------------------------------------------------------------------------------------------------------------------
# the cases: what the GPU test encodes and the CPU test checks the properties of
# ---------------------------------------------------------------------------------------------------------------------
class Case:
    """One input: pcm [B][n][ch] and its setting - `rates` float32 [B][2] (the per-stream table: -quality for VBR), or
    mode / p0 / p1 for the whole batch.  refs / units: the oracle's results and the counts, per stream."""

    def __init__(self, name, bs, ch, pcm, rates=None, mode=0, p0=None, p1=0.0, rate=RATE):
        self.name, self.bs, self.ch, self.pcm, self.rate = name, bs, ch, np.ascontiguousarray(pcm, np.float32), rate
        self.rates = None if rates is None else np.ascontiguousarray(rates, np.float32)
        self.mode, self.p0, self.p1 = mode, p0, p1
        self.B, self.K = self.pcm.shape[0], self.pcm.shape[1] // bs
        self._refs = self._units = None

    def setting(self, s):
        if self.rates is None:
            return self.mode, float(self.p0), float(self.p1)
        r, a = (float(v) for v in self.rates[s])
        return (0, -r, 0.0) if r < 0 else ((2, r, a) if a > 0 else (1, r, 0.0))

    @property
    def refs(self):
        if self._refs is None:
            done = {}                                       # (streams of a tiled batch share their reference)
            self._refs = []
            for s in range(self.B):
                key = (self.pcm[s].tobytes(), self.setting(s))
                if key not in done:
                    done[key] = oracle_encode_debug(self.pcm[s], self.bs, self.rate, *self.setting(s))
                self._refs.append(done[key])
        return self._refs

    @property
    def units(self):
        if self._units is None:
            done = {}
            self._units = []
            for r in self.refs:
                if id(r) not in done:
                    done[id(r)] = stream_units(r, self.ch, self.bs)
                self._units.append(done[id(r)])
        return self._units

    def predicted(self, plan, every=0, direct=True, k0=0, K=None):
        """([B][K] flags, [B][K] "on the exact path") of the call over blocks k0 .. k0 + K of every stream.  every:
        ulcx_encoder_debug_force_exact, 0 or 1 here.  A block is on the exact path if it keeps anything and its tie group
        straddles the cut or the hook sends it there.  direct: ULCX_DIRECT_PACK is not 0."""
        K = K or self.K
        exact = np.array([[int(self.refs[s]["nout"][k0 + k]) > 0 and (every == 1 or straddles(self.refs[s], k0 + k)) for k in range(K)] for s in range(self.B)])
        single = exact_trip_is_single(self.B * K, int(exact.sum()), self.ch)
        return np.array([[predict_flags(self.units[s][k0 + k], plan, self.ch, exact=bool(exact[s, k]), direct=direct and (single or not exact[s, k]))
                          for k in range(K)] for s in range(self.B)], np.int32), exact


N_BLOCKS = 6
BOUNDARY_BLOCK = 3                                         # the block of the boundary streams whose kept count is solved for


@functools.lru_cache(maxsize=None)
def boundary_case(bs, cap):
    """bs x 1, white noise, two streams of the same samples: VBR qualities at which block BOUNDARY_BLOCK keeps exactly `cap`
    and `cap + 1` coefficients (mono, un-decimated: the unit is the block, nK = nout)."""
    pcm = noise_pcm(bs * N_BLOCKS, 1, 1)
    qs = [quality_for_nout(pcm, bs, BOUNDARY_BLOCK, want) for want in (cap, cap + 1)]
    assert None not in qs, (bs, cap, qs)
    return Case(f"boundary {bs}x1 at {cap}", bs, 1, np.stack([pcm, pcm]), rates=[[-q, 0.0] for q in qs])


@functools.lru_cache(maxsize=None)
def full_never_fails_case():
    bs = 1024
    return Case("1024x1 white noise q100", bs, 1, np.stack([noise_pcm(bs * N_BLOCKS, 1, 11 + s) for s in range(2)]), mode=0, p0=100.0)


@functools.lru_cache(maxsize=None)
def no_retry_case(bs):
    """Geometries with one launch of the wave writer (the full tier is no larger than the small one).  512: white noise with
    everything kept - more than 128 zones in 512 coefficients.  256: tones two bins apart, alternating 1 and 1/32."""
    n = bs * N_BLOCKS
    pcm = noise_pcm(n, 1, 2) if bs == 512 else comb_pcm(n, bs, 4, 2, (bs - 16) // 2, (1.0, 1.0 / 32.0))
    return Case(f"no retry tier {bs}x1", bs, 1, pcm[None], mode=0, p0=100.0)


Z_QUALITY, N_QUALITY = 78.0, 76.25


@functools.lru_cache(maxsize=None)
def single_cause_case():
    """2048 x 1, stream 0: Z alone, stream 1: N alone"""
    bs = 2048
    n = bs * N_BLOCKS
    return Case("Z alone, N alone", bs, 1, np.stack([z_comb(n, bs), n_comb(n, bs)]), rates=[[-Z_QUALITY, 0.0], [-N_QUALITY, 0.0]])


@functools.lru_cache(maxsize=None)
def gap_case(bs):
    """G: bs x 1 at quality 20.  8192: floors 1e-3 and 2e-4, gaps of 57 and 59 run-code nybbles.  4096: floor 1e-3 - a block with a
    gap of exactly 32 nybbles, the most a wave holds - and 2e-4 (36)."""
    n = bs * N_BLOCKS
    return Case(f"G {bs}x1", bs, 1, np.stack([sparse_pcm(n, RATE, 1, 1e-3), sparse_pcm(n, RATE, 1, 2e-4)]), mode=0, p0=20.0)


STEREO_KINDS = ("neither", "channel 0 only", "channel 1 only", "both")


def stereo_kind(units, small):
    over = [any(causes(u, small) for u in units if u["ch"] == c) for c in (0, 1)]
    return STEREO_KINDS[int(over[0]) + 2 * int(over[1])]


def _stereo_streams(n):
    rng = np.random.default_rng([0x57E2E0, 5])
    dense, faint = 0.25 * rng.standard_normal(n), 0.001 * rng.standard_normal(n)
    t = np.arange(n) / RATE
    x = sum(a * np.sin(2 * np.pi * f * t + p) for f, a, p in ((440.0, 0.3, 0.1), (1234.5, 0.2, 1.0), (3300.0, 0.1, 2.0), (7000.0, 0.05, 0.5)))
    y = sum(a * np.sin(2 * np.pi * f * t + p) for f, a, p in ((523.0, 0.1, 0.7), (2500.0, 0.05, 1.3)))
    return np.stack([stereo_from_mid_side(x, y),             # tonal: neither channel over
                     stereo_from_mid_side(dense, faint),     # R = L plus a faint floor: the coded mid channel is the dense one
                     stereo_from_mid_side(faint, dense),     # R = -L plus a faint floor: the side channel
                     noise_pcm(n, 2, 3)])                    # independent dense channels: both


STEREO_QUALITY = 85.0


@functools.lru_cache(maxsize=None)
def stereo_case(tile=1, n_blocks=N_BLOCKS):
    """2048 x 2 at quality 85: four streams, one per kind of un-decimated block; tile > 1 repeats them (the exact path at scale)"""
    bs = 2048
    return Case(f"stereo hand-over x{tile}", bs, 2, np.tile(_stereo_streams(bs * n_blocks), (tile, 1, 1)), mode=0, p0=STEREO_QUALITY)


@functools.lru_cache(maxsize=None)
def decimated_case(bs):
    """bs x 2: one strong burst late in block 3 of a dense noise bed.  The block that decimates for it has one unit over a
    small capacity, and that unit is not the first of its channel."""
    bed, q = (0.1, 90.0) if bs == 2048 else (0.05, 85.0)
    return Case(f"decimated {bs}x2", bs, 2, burst_pcm(bs * N_BLOCKS, 2, bs, 3, 1, bed=bed)[None], mode=0, p0=q)


RATE_SETTINGS = {(1, 1): (1, 256.0, 0.0), (1, 2): (2, 320.0, 1.0), (2, 1): (1, 512.0, 0.0), (2, 2): (2, 640.0, 1.0)}     # (ch, mode) -> mode, kbps, AvgComplexity


@functools.lru_cache(maxsize=None)
def rate_case(ch, mode):
    """2048 x ch white noise under CBR / ABR at a rate whose final nout puts a unit above 1024 kept coefficients"""
    bs = 2048
    m, p0, p1 = RATE_SETTINGS[(ch, mode)]
    return Case(f"rate search 2048x{ch} mode {m}", bs, ch, np.stack([noise_pcm(bs * N_BLOCKS, ch, 7 + s) for s in range(2)]), mode=m, p0=p0, p1=p1)


LADDER_DENSE, LADDER_SPARSE = 90.0, 30.0


@functools.lru_cache(maxsize=None)
def ladder_case(q):
    return Case(f"ladder rung q{q:g}", 2048, 2, _stereo_streams(2048 * N_BLOCKS), mode=0, p0=q)


# ---------------------------------------------------------------------------------------------------------------------
# the capacities enc_plan (csrc/ulcx_enc.hip) gives, by BlockSize: what ulcx_encoder_debug_writer_plan must report
# ---------------------------------------------------------------------------------------------------------------------
SMALL, MEDIUM, FULL = (512, 128, 1280), (1024, 512, 4096), (2048, 1024, 8256)


def expected_plan(bs):
    """full: {BS, BS/2, 4*BS + 64}, halved (nybbles: / 2 + 32) until four waves fit 150 KB of LDS - from BlockSize 2048 on it
    is 2048 / 1024 / 8256.  have_full: the full tier is larger than the small one; have_mid: the medium one smaller than the full."""
    full = {256: (256, 128, 1088), 512: (512, 256, 2112), 1024: (1024, 512, 4160)}.get(bs, FULL)
    return dict(small=SMALL, medium=MEDIUM, full=full, have_mid=MEDIUM[0] < full[0], have_full=full[0] > SMALL[0])
