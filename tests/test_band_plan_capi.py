"""The Bark band tables over the sample-rate axis, on the CPU: ulcx_debug_band_plan (the code ulcx_encoder_create runs, no
device) against edges formed from the oracle's helpers - orc_bark_to_freq and orc_freq_to_line, pinned to the reference by
test_oracle_pinned.py - with floor, ceil and the clamps of ulcEncoder_Psyopt.c:109-116 and :198-205 in numpy.  Equality is
exact: both sides call this machine's libm.  Then what k_bark_uniform relies on wherever the ring is not 0, the hook's own
count against a recount, and the census: every (BlockSize, RateHz) of tests/test_gpu_rate_axis.py is in the ring class its
test is named for.  That last test is what keeps a GPU case from passing on the wrong kernels."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ulc-codec_amd"))
import rate_axis_testlib as R
from ulc_testlib import oracle

LIB = os.path.join(ROOT, "ulc-codec_amd", "libulc_amd.so")
NAMES = ("ulcx_debug_band_plan", "ulcx_debug_band_events", "ulcx_encoder_debug_plan")
NBARK, MAX_SUB, EVENTS = 25, 4, 52
BLOCK_SIZES = [256 << i for i in range(8)]                  # 256 .. 32768
NAMED_RATES = [1, 100, 1000, 4000, 8000, 11025, 12000, 16000, 22050, 24000, 32000, 44100, 48000, 64000, 88200, 96000, 176400, 192000,
               384000, 768000]
RATES = NAMED_RATES + [int(r) for r in np.random.default_rng(0xBA2C).integers(1, 768001, 200)]
OFFSETS = ((0.0, 2.0), (-0.75, 0.25))                       # noise: Psyopt.c:198-199; masking: :109-110


@pytest.fixture(scope="module")
def amd():
    if not os.path.exists(LIB):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "ulc-codec_amd"), "-j8"], stdout=subprocess.DEVNULL)
    import ulc_amd
    return ulc_amd


@pytest.fixture(scope="module")
def plans(amd):
    """(edges [2][4][2][25], most, ring) of every (BlockSize, RateHz) of the sweep, from the hook."""
    return {(bs, r): amd.band_plan(bs, r) for bs in BLOCK_SIZES for r in sorted(set(RATES))}


_freqs = {}
_edges = {}


def oracle_edges(n_lines, rate):
    """[noise|masking][beg|end][25] for a sub-block of n_lines lines: the oracle's helpers per band, the rest in numpy."""
    key = (n_lines, rate)
    if key not in _edges:
        lib = oracle()
        if not _freqs:
            for lo, hi in OFFSETS:
                for off in (lo, hi):
                    _freqs[off] = [lib.orc_bark_to_freq(float(np.float32(b) + np.float32(off))) for b in range(NBARK)]
        nyq = float(np.float32(rate) * np.float32(0.5))
        out = np.zeros((2, 2, NBARK), np.int64)
        for t, (lo, hi) in enumerate(OFFSETS):
            x0 = np.array([lib.orc_freq_to_line(f, nyq, n_lines) for f in _freqs[lo]], np.float32)
            x1 = np.array([lib.orc_freq_to_line(f, nyq, n_lines) for f in _freqs[hi]], np.float32)
            out[t, 0] = np.clip(np.floor(x0).astype(np.int64), 0, n_lines - 1)
            out[t, 1] = np.clip(np.ceil(x1).astype(np.int64), 0, n_lines)
        _edges[key] = out
    return _edges[key]


def open_counts(beg, end, n):
    """[line][band]: the bands open at a line of one table - lower edge passed, upper edge not yet, both inclusive (the event list
    has a band of no lines open and close at one line).  Only at the lines where a band opens: nowhere else can the set grow."""
    pos = np.unique(beg)[:, None]
    assert pos.max() <= n
    return (beg[None, :] <= pos) & (pos <= end[None, :])


def test_hooks_are_exported_and_bound(amd):
    lib = amd.lib()
    for n in NAMES:
        assert hasattr(lib, n) and n in amd.EXPORTS, n
    assert hasattr(amd, "band_plan") and hasattr(amd, "band_events") and hasattr(amd.BatchEncoder, "plan")
    assert (amd.N_BARK, amd.MAX_SUB, amd.BARK_EVENTS) == (NBARK, MAX_SUB, EVENTS)


def test_hooks_refuse_what_no_encoder_has(amd):
    lib = amd.lib()
    lib.ulcx_last_error.restype = C.c_char_p
    edges = (C.c_int16 * (2 * MAX_SUB * 2 * NBARK))()
    ev = (C.c_uint32 * (2 * MAX_SUB * EVENTS))()
    plan = (C.c_int32 * 8)()
    band = C.CFUNCTYPE(C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p)(("ulcx_debug_band_plan", lib))
    events = C.CFUNCTYPE(C.c_int, C.c_int, C.c_int, C.c_void_p)(("ulcx_debug_band_events", lib))
    oplan = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p)(("ulcx_encoder_debug_plan", lib))
    for bs, rate in ((2048, 0), (2048, -44100), (128, 44100), (65536, 44100), (3000, 44100), (0, 44100)):
        assert band(bs, rate, C.addressof(edges), None, None) == -1 and lib.ulcx_last_error().decode().startswith("ulcx_debug_band_plan:")
        assert events(bs, rate, C.addressof(ev)) == -1 and lib.ulcx_last_error().decode().startswith("ulcx_debug_band_events:")
    assert band(2048, 44100, None, None, None) == -1 and events(2048, 44100, None) == -1
    assert oplan(None, C.addressof(plan)) == -1 and lib.ulcx_last_error().decode().startswith("ulcx_encoder_debug_plan:")
    assert oplan(C.c_void_p(16), None) == -1                 # (never dereferenced: the array is checked with the object)
    assert not any(edges) and not any(ev) and not any(plan)
    assert band(2048, 44100, C.addressof(edges), None, None) == 0 and any(edges)      # most and ring are optional


def test_edges_equal_the_oracle_helpers_at_every_size_and_rate(plans):
    bad = []
    for (bs, rate), (edges, most, ring) in plans.items():
        for d in range(MAX_SUB):
            want = oracle_edges((bs >> d) // 2, rate)
            if not np.array_equal(edges[:, d].astype(np.int64), want):
                bad.append((bs, rate, d))
    assert not bad, f"{len(bad)} tables differ from the oracle's edges, first (BlockSize, RateHz, d): {bad[:5]}"
    assert len(plans) == len(BLOCK_SIZES) * len(set(RATES)) and len(set(RATES)) >= 215


def test_edges_are_ordered_and_inside_the_subblock(plans):
    """Holds at every size and rate, ring or not: what the event list's builder and the ring's sizing test for."""
    for (bs, rate), (edges, most, ring) in plans.items():
        e = edges.astype(np.int64)
        for d in range(MAX_SUB):
            n = (bs >> d) // 2
            for t in range(2):
                beg, end = e[t, d, 0], e[t, d, 1]
                assert (np.diff(beg) >= 0).all() and (np.diff(end) >= 0).all(), (bs, rate, t, d)
                assert (0 <= beg).all() and (beg <= end).all() and (end <= n).all(), (bs, rate, t, d)


def test_most_and_ring_equal_a_recount(plans):
    seen = set()
    for (bs, rate), (edges, most, ring) in plans.items():
        e = edges.astype(np.int64)
        n = bs // 2
        count = max(int(open_counts(e[t, 0, 0], e[t, 0, 1], n).sum(axis=1).max()) for t in range(2))
        assert most == count, (bs, rate, most, count)
        assert ring == (4 if count <= 4 else 8 if count <= 8 else 0), (bs, rate, most, ring)      # (BlockSize / 2 is a multiple of 32 from 256 up)
        seen.add((ring, count == ring))
    assert seen >= {(0, False), (4, False), (4, True), (8, False), (8, True)}, seen


def test_ring_never_holds_two_open_bands_in_one_slot(plans):
    """What k_bark_uniform relies on wherever the ring is not 0, on the full-size tables it walks: at no line more bands open
    than the ring holds, and no two bands open at one line in the same snapshot slot b & (ring - 1)."""
    n_ring = 0
    for (bs, rate), (edges, most, ring) in plans.items():
        if not ring:
            continue
        n_ring += 1
        e = edges.astype(np.int64)
        for t in range(2):
            op = open_counts(e[t, 0, 0], e[t, 0, 1], bs // 2)                     # [line][band]
            assert op.sum(axis=1).max() <= ring, (bs, rate, t)
            slots = np.zeros((op.shape[0], ring), np.int64)
            for b in range(NBARK):
                slots[:, b & (ring - 1)] += op[:, b]
            assert slots.max() <= 1, (bs, rate, t)
    assert n_ring > 500


def test_event_lists_are_the_edges_in_line_order(amd, plans):
    """The list of every table fits ULCX_BARK_EVENTS, holds every edge once in line order - at equal lines lower edges in front
    of upper edges - then the end of the sub-block, then padding."""
    for bs in BLOCK_SIZES:
        for rate in NAMED_RATES + RATES[len(NAMED_RATES)::8]:
            ev = amd.band_events(bs, rate)
            e = plans[(bs, rate)][0].astype(np.int64)
            for t in range(2):
                for d in range(MAX_SUB):
                    n = (bs >> d) // 2
                    want = sorted([(int(e[t, d, 0, b]), 0, b) for b in range(NBARK)] + [(int(e[t, d, 1, b]), 1, b) for b in range(NBARK)])
                    assert len(want) + 1 <= EVENTS
                    words = [p | k << 16 | b << 24 for p, k, b in want] + [n | 2 << 16]
                    words += [0xffff | 3 << 16] * (EVENTS - len(words))
                    assert [int(w) for w in ev[t, d]] == words, (bs, rate, t, d)


def test_census_every_gpu_case_is_in_its_ring_class(plans, amd):
    """The (BlockSize, RateHz) of every case of tests/test_gpu_rate_axis.py, by the class its test is named for: (ring, most bands
    open at one line), most == None where the ring alone is the class.  On this libm every rate the cases were drawn up with is
    in its class as it stands; were one not, the nearest rate that is takes its place in rate_axis_testlib, found here."""
    wrong = []
    for bs, rate, cls in R.ALL_CLASSED:
        edges, most, ring = plans[(bs, rate)] if (bs, rate) in plans else amd.band_plan(bs, rate)
        if not R.in_class(most, ring, cls):
            wrong.append((bs, rate, cls, (ring, most)))
    assert not wrong, f"(BlockSize, RateHz, class wanted, (ring, most) found): {wrong}"
    classes = {cls for _, _, cls in R.ALL_CLASSED}
    assert {(0, None), (0, 9), (8, 7), (8, 8), (4, 4), (8, None), (4, None)} <= classes


def test_the_batch_comparison_notices_each_kind_of_difference():
    """rate_axis_testlib.compare_call on the oracle's own results, tiled: equal as they stand; one window code, one bit of a
    complexity, one size, one byte in the middle of a block and a block's last byte are each
    reported; what lies behind a block's last byte is not looked at."""
    bs, ch, rate, K = 256, 2, 96000, 6
    distinct = R.distinct_streams(bs, ch, rate, 2 * K, seed=1)
    refs = R.oracle_refs(distinct, bs, rate, R.VBR50, 2 * ch * bs + 16)
    pcm, src = R.tiled(distinct, 12, seed=2)
    assert pcm.shape == (12, 2 * K * bs, ch) and sorted(set(src)) == list(range(5)) and not np.array_equal(src, np.sort(src))

    def results():
        sl = slice(K, 2 * K)
        return [np.stack([refs[i][f][sl] for i in src]).copy() for f in ("out", "bits", "wc", "cplx")]

    R.compare_call(results(), refs, src, K, "as is")
    with pytest.raises(AssertionError, match="WindowCtrl"):
        R.compare_call(results(), refs, src, 0, "the other call's blocks")
    s, k = 9, 5
    nb = int(results()[1][s, k]) // 8
    for what, field, at, flip in (("WindowCtrl", 2, (3, 1), 0x10), ("size", 1, (5, 2), 4), ("bytes differ", 0, (7, 3, 2), 0x40),
                                  ("bytes differ", 0, (s, k, nb - 1), 0x80)):
        r = results()
        r[field][at] ^= flip
        with pytest.raises(AssertionError, match=what):
            R.compare_call(r, refs, src, K, "changed")
    r = results()
    r[3].view(np.uint32)[4, 4] ^= 1
    with pytest.raises(AssertionError, match="BlockComplexity"):
        R.compare_call(r, refs, src, K, "changed")
    r = results()
    r[0][s, k, nb:] ^= 0xFF
    R.compare_call(r, refs, src, K, "behind the last byte")
