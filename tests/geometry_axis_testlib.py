"""The geometry axis: what tests/test_geometry_axis_capi.py (CPU) and tests/test_gpu_geometry_axis.py share.

The encoder picks its kernels from (nChan, BlockSize) alone ("Geometry classes").  classes() restates those picks in
plain Python, every rule beside the source lines it restates; CASES holds the smallest shape of every selection class plus
one with more than two channels wherever the class admits one, and KINDS says under which call kinds a case runs.  The CPU test
asserts that every case is in the class it is listed under, that every class is reached by every kind that can reach it,
and that the oracle's run of a case has the blocks the case is there for; the GPU test asserts the model again from the object it
opened (ulcx_encoder_debug_plan) and compares every call with the oracle alone, bit for bit.

A batch is 7 streams (the five of rate_axis_testlib.distinct_streams, digital silence, one stream at 2^-14 of full scale), all
on the PCM16 grid, in two calls of 3 and 6 blocks on one object: state carries, the calls have 21 and 42 blocks - the last
workgroup of a wave selection (four blocks each) has idle waves - and the 6-block call takes the chunked front end."""
import functools
import numpy as np
from ulc_testlib import oracle_decode_stream
from rates_testlib import OracleStream, mode_of
from rate_axis_testlib import distinct_streams, decimated, _grid16

RATE = 44100
B = 7
CALLS = (3, 6)                      # blocks per call
NBLK = sum(CALLS)
KMAX = max(CALLS)
SILENT, QUIET = 5, 6                # rows of streams() behind the five distinct ones

ULCX_HEAP_LDS_BYTES = 128 * 1024    # ulc-codec_amd/csrc/ulcx_internal.h:16
ULCX_LDS_LIMIT = 160 * 1024         # ulc-codec_amd/csrc/ulcx_internal.h:193

SEL = ("W4", "W8", "W16", "W32", "W64", "W64c", "W128", "P128", "G")
XF = ("X2", "X1", "Xn", "Xn8192", "XB")
WC = ("fused", "split")
GAP = ("on", "off_by_size", "off_by_channels")
HEAP = ("lds", "hbm")


def classes(bs, ch):
    """dict(sel, xf, wc, gap, heap) of an encoder of BlockSize bs with ch channels."""
    n = ch * bs
    # ulcx_enc.hip:67-82 select_fn_pass: R = C * BS / 64 keys per lane; 128 -> k_select_pair for a pair (ulcx_enc.hip:249: stereo,
    # R == 128), else k_select_wave<128, 0>; 64 -> <64, 11> for lgBS == 11 (stereo 2048), else <64, 0>; 32, 16, 8, 4 -> <R, 0>;
    # everything else NULL.  ulcx_enc.hip:248: selWave only for those six R, and they must be exact (N / 64 truncates: 256 x 3 has
    # N = 768, R = 12, not a wave size) - ulcx_enc.hip:323 launches the generic k_select otherwise.
    r = n // 64
    if r == 128:
        sel = "P128" if ch == 2 else "W128"
    elif r == 64:
        sel = "W64c" if bs == 2048 else "W64"
    elif r in (4, 8, 16, 32):
        sel = "W%d" % r
    else:
        sel = "G"
    # ulcx_enc.hip:57-61 xf_fn_in: above BlockSize 8192 k_xf_big / k_xfa_big whatever the channel count; C == 2 k_xf<true>; every
    # other count k_xf<false>.  ulcx_enc_xf.hip:219-220: line energies in LDS only for C > 2, and then the twiddles stay in global
    # memory when 16 * (BS + BS / 16) + 4 * BS + 32 bytes exceed the LDS limit (ulcx_enc.hip:32-33): BlockSize 8192.
    if bs > 8192:
        xf = "XB"
    elif ch == 2:
        xf = "X2"
    elif ch == 1:
        xf = "X1"
    elif 16 * (bs + (bs >> 4)) + 4 * bs + 32 > ULCX_LDS_LIMIT:
        xf = "Xn8192"
    else:
        xf = "Xn"
    # ulcx_enc.hip:138: k_wc_ef for C == 2, k_wc_energy + k_wc_forward for every other count
    wc = "fused" if ch == 2 else "split"
    # ulcx_api.cpp:291: useGapSums = (C * BS <= 16384 && nChan <= 16).  A geometry that fails both tests is listed by its size.
    gap = "off_by_size" if n > 16384 else "off_by_channels" if ch > 16 else "on"
    # ulcx_enc.hip:251, ulcx_api.cpp:309: the exact path's heap in LDS while C * BS * 8 <= ULCX_HEAP_LDS_BYTES
    heap = "lds" if n * 8 <= ULCX_HEAP_LDS_BYTES else "hbm"
    return dict(sel=sel, xf=xf, wc=wc, gap=gap, heap=heap)


def plan_fields(bs, ch):
    """What ulcx_encoder_debug_plan reports of the model (fields 2, 3 and 6)."""
    c = classes(bs, ch)
    return dict(use_gap_sums=int(c["gap"] == "on"), heap_in_lds=int(c["heap"] == "lds"), sel_pair=int(c["sel"] == "P128"))


# (BlockSize, channels, the selection class the case is listed under)
CASES = [
    (256, 1, "W4"),
    (512, 1, "W8"), (256, 2, "W8"),
    (1024, 1, "W16"), (256, 4, "W16"),
    (2048, 1, "W32"), (256, 8, "W32"),
    (4096, 1, "W64"), (1024, 4, "W64"), (256, 16, "W64"),        # 256 x 16: gap sums on, at their channel limit
    (2048, 2, "W64c"),
    (8192, 1, "W128"), (2048, 4, "W128"), (256, 32, "W128"),      # 256 x 32: off_by_channels, heap in LDS
    (4096, 2, "P128"),
    (256, 3, "G"), (256, 17, "G"),                                # 256 x 17: the first off_by_channels
    (2048, 9, "G"),                                               # off_by_size, heap in the object's scratch, Xn
    (8192, 3, "G"),                                               # Xn8192
    (16384, 1, "G"),                                              # XB
    (256, 255, "G"),                                              # the ABI's last channel count
]

# every case runs these; "decode": the oracle's VBR 50 bytes through BatchDecoder
EVERY_CASE = ("vbr", "search", "table", "ladder", "decode")
# one geometry of each (gap, heap) pair that exists
EXACT = [(256, 16), (256, 32), (2048, 9)]
# one geometry of each xf class and each wc class, and the first channel count without gap sums
FRONT = [(256, 2), (256, 1), (256, 3), (8192, 3), (16384, 1), (256, 17)]
KINDS = {(bs, ch): EVERY_CASE + (("exact",) if (bs, ch) in EXACT else ()) + (("analyse", "pcm16") if (bs, ch) in FRONT else ())
         for bs, ch, _ in CASES}


def cases_of(kind):
    return [(bs, ch) for bs, ch, _ in CASES if kind in KINDS[(bs, ch)]]


def case_id(c):
    return "%dx%d" % (c[0], c[1])


# ---------------------------------------------------------------------------
# rate settings, in the reference tool's convention (RateKbps, AvgComplexity): RateKbps < 0 is VBR at quality -RateKbps
# ---------------------------------------------------------------------------
VBR1, VBR50, VBR100 = (-1.0, 0.0), (-50.0, 0.0), (-100.0, 0.0)
CBR32 = (32.0, 0.0)
ABR96 = (96.0, 0.45)
ABR64, ABR128 = (64.0, 0.2), (128.0, 0.5)


def cbr_of(ch):
    """48 kbps per channel pair"""
    return (48.0 * ((ch + 1) // 2), 0.0)


def table_of(ch):
    """The per-stream table, row s for stream s: the two synth_pcm streams under CBR 32 and VBR 100 (the rows the census compares),
    digital silence in a rate search, the quiet stream under VBR 1."""
    return [CBR32, VBR100, ABR128, VBR50, cbr_of(ch), ABR64, VBR1]


TABLE_CBR_ROW, TABLE_VBR100_ROW = 0, 1


def ladder_of(ch):
    return [VBR50, cbr_of(ch), VBR100]


def scalar(setting):
    """(mode, p0, p1) of the scalar calls"""
    return mode_of(setting)


# ---------------------------------------------------------------------------
# the streams and their oracle runs: computed once per process, shared by every test, never written to
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def streams(bs, ch):
    """[7][9 * bs][ch] float32 on the PCM16 grid."""
    n = NBLK * bs
    five = distinct_streams(bs, ch, RATE, NBLK, seed=bs + ch)
    silent = np.zeros((1, n, ch), np.float32)
    # full-scale white noise times 2^-14: samples of -2 .. 2 PCM16 steps in every channel
    quiet = _grid16(np.random.default_rng([0x9E7, bs, ch]).uniform(-1.0, 1.0, (n, ch)) * 2.0 ** -14)[None]
    pcm = np.ascontiguousarray(np.concatenate([five, silent, quiet]), np.float32)
    pcm.setflags(write=False)
    return pcm


@functools.lru_cache(maxsize=None)
def oracle_stream(bs, ch, s, setting):
    """Stream s of the case encoded by the oracle under one setting: a tuple of 9 per-block dicts (bytes, bits, wc, cplx, nout,
    keep), as rates_testlib.OracleStream gives them."""
    o = OracleStream(ch, bs, RATE)
    x = streams(bs, ch)[s]
    blocks = tuple(o.block(x[k * bs:(k + 1) * bs], setting) for k in range(NBLK))
    o.close()
    return blocks


def oracle_rows(bs, ch, settings):
    """refs[s][k] for the batch with settings[s] on stream s (one setting: the same on every stream)."""
    if isinstance(settings, tuple):
        settings = [settings] * B
    return [oracle_stream(bs, ch, s, tuple(float(v) for v in settings[s])) for s in range(B)]


@functools.lru_cache(maxsize=None)
def oracle_decoded(bs, ch):
    """(blocks uint8 [7][9][slot], pcm float32 [7][9 * bs][ch], bits int32 [7][9]): the oracle's VBR 50 streams and its own decode
    of them."""
    slot = 2 * ch * bs + 16
    blocks = np.zeros((B, NBLK, slot), np.uint8)
    pcm = np.zeros((B, NBLK * bs, ch), np.float32)
    bits = np.zeros((B, NBLK), np.int32)
    for s, ref in enumerate(oracle_rows(bs, ch, VBR50)):
        for k, o in enumerate(ref):
            blocks[s, k, :o["bytes"].size] = o["bytes"]
        rc, pcm[s], bits[s] = oracle_decode_stream(blocks[s], ch, bs)
        assert rc == 0, f"{bs} x {ch} stream {s}: the oracle refuses its own stream ({rc})"
    for a in (blocks, pcm, bits):
        a.setflags(write=False)
    return blocks, pcm, bits


def call_spans():
    """[(call, first block, blocks)]"""
    out, k0 = [], 0
    for j, K in enumerate(CALLS):
        out.append((j, k0, K))
        k0 += K
    return out


# ---------------------------------------------------------------------------
# what the oracle's run of a case must hold (the census); every function returns the numbers it judged by
# ---------------------------------------------------------------------------
def live_block_kinds(refs):
    """(decimated, un-decimated) blocks that keep coefficients"""
    dec = np.array([bool(decimated(o["wc"])) for r in refs for o in r if o["nout"] > 0])
    return int(dec.sum()), int((~dec).sum())


def kept_per_stream(refs):
    """blocks with nOutCoef > 0, per stream"""
    return [sum(1 for o in r if o["nout"] > 0) for r in refs]


def blocks_compared(kind, ch):
    """Blocks a GPU test of this kind holds against the oracle for one case."""
    per = B * NBLK
    return {"vbr": per, "search": 2 * per, "table": per, "ladder": len(ladder_of(ch)) * per, "decode": per, "exact": 3 * per,
            "analyse": per, "pcm16": 2 * per}[kind]


# ---------------------------------------------------------------------------
# the comparison: sizes, WindowCtrl, BlockComplexity bit patterns and bytes, kept sets where the taps give them; no tolerance
# ---------------------------------------------------------------------------
def compare_call(res, refs, call, k0, what, taps=None, bs=None):
    """One call's (out [B][K][slot], bits [B][K], wc [B][K], cplx [B][K]) against blocks [k0, k0 + K) of refs[s]; taps: the keep
    and nout parts of debug_fetch behind that call (bs: the BlockSize, to name the channel of a differing coefficient)."""
    out, bits, wc, cplx = res
    nB, K = bits.shape
    assert nB == len(refs)
    for s in range(nB):
        for k in range(K):
            o = refs[s][k0 + k]
            tag = f"{what}: stream {s} call {call} block {k} (block {k0 + k} of the stream)"
            assert wc[s, k] == o["wc"], f"{tag}: WindowCtrl {wc[s, k]:#x} != {o['wc']:#x}"
            assert cplx[s, k].view(np.uint32) == o["cplx"].view(np.uint32), f"{tag}: BlockComplexity {cplx[s, k]!r} != {o['cplx']!r}"
            assert bits[s, k] == o["bits"], f"{tag}: size {bits[s, k]} != {o['bits']} bits"
            assert bits[s, k] > 0 and bits[s, k] % 8 == 0, f"{tag}: {bits[s, k]} bits are no whole bytes"
            got = out[s, k, :bits[s, k] // 8]
            if not np.array_equal(got, o["bytes"]):
                raise AssertionError(f"{tag}: bytes differ from byte {int(np.argmax(got != o['bytes']))} of {got.size}")
            if taps is not None:
                assert taps["nout"][s, k] == o["nout"], f"{tag}: nOutCoef {taps['nout'][s, k]} != {o['nout']}"
                if not np.array_equal(taps["keep"][s, k], o["keep"]):
                    i = int(np.argmax(taps["keep"][s, k] != o["keep"]))
                    raise AssertionError(f"{tag}: kept set differs from coefficient {i}" + (f" (channel {i // bs})" if bs else ""))


def compare_series(wc, cplx, refs, call, k0, what):
    """An analysis call's (wc [B][K], cplx [B][K]) against the oracle's."""
    nB, K = wc.shape
    for s in range(nB):
        for k in range(K):
            o = refs[s][k0 + k]
            tag = f"{what}: stream {s} call {call} block {k} (block {k0 + k} of the stream)"
            assert wc[s, k] == o["wc"], f"{tag}: WindowCtrl {wc[s, k]:#x} != {o['wc']:#x}"
            assert cplx[s, k].view(np.uint32) == o["cplx"].view(np.uint32), f"{tag}: BlockComplexity {cplx[s, k]!r} != {o['cplx']!r}"
