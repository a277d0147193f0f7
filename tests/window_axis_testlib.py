"""The window axis: what tests/test_window_axis_capi.py (CPU) and tests/test_gpu_window_axis.py share.

Window control gives every block one WindowCtrl code - un-decimated 0x10, or one of eight transient positions times an overlap
scale - and that code, with the codes of the block in front and the block behind, picks what the transform does (DESIGN.md,
"Window classes").  codes() restates which codes k_wc_decide can emit at a BlockSize, block_class() which form of the transform
a block takes, front_plan() where a call's launch cuts its window-control steps and transform chunks; every rule stands beside
the source lines it restates.  designed() builds an input with one event per chosen block; TABLE holds, per geometry, one
parameter set per code that search() found with the oracle (run by hand: python tests/window_axis_testlib.py), and nothing is
searched while the tests run.  The CPU test holds the oracle's runs of the table's streams against the model and counts what
they reach; the GPU test compares every call of the same streams with the oracle, bit for bit."""
import functools
import sys
import numpy as np
from ulc_testlib import oracle_encode_stream, oracle_encode_debug, oracle_decode_stream

RATE = 44100
UNDEC = 0x10

# the smallest geometry of every transform and window-control class (tests/geometry_axis_testlib.py: X2 / X1 / Xn / Xn8192 / XB,
# fused / split), the two xf_fast sizes, and the largest BlockSize
GEOMETRIES = [(256, 2), (256, 1), (512, 3), (1024, 2), (2048, 2), (4096, 2), (2048, 1), (8192, 3), (16384, 1), (32768, 1)]
FULL_SET_UP_TO = 4096               # every code of codes(bs) must be reached up to here; above: every position and every scale


def geo_id(g):
    return "%dx%d" % g


# ---------------------------------------------------------------------------
# the model
# ---------------------------------------------------------------------------
def lg(bs):
    return bs.bit_length() - 1


def n_seg(bs):
    """Segments the decision loop compares.  ulcx_enc_wc.hip:394-395: nSeg = 8, and below BlockSize 512 (log2sub = lgBS - 3 < 6)
    nSeg >>= 6 - log2sub: 4 at BlockSize 256."""
    sub = lg(bs) - 3
    return 8 >> max(0, 6 - sub)


def max_scale(bs):
    """The largest overlap scale.  ulcx_enc_wc.hip:391-397: log2sub = max(lgBS - 3, 6), and the loop's first pass makes it one
    more; the loop never runs a second pass (a pass that does not break at :416 leaves ratio = maxRatio >= ln 2, which fails the
    test ratio < ln 2 of :419).  :426-427: scale <= 7 and log2sub - scale >= 6."""
    return min(7, max(lg(bs) - 3, 6) + 1 - 6)


def codes(bs):
    """Every WindowCtrl k_wc_decide can emit at BlockSize bs.
    ulcx_enc_wc.hip:416 a first pass that breaks leaves decimation = 1, ratio = 0: :423 gives 0x10, the only un-decimated code;
    :417 otherwise decimation = nSeg + maxSeg (the position digit: 8 .. 15, at BlockSize 256 4 .. 7) and ratio >= ln 2, so
    ratio * log2(e) >= 1 and :426 rounds to scale >= 1 - there is no scale 0 and ratio never lies in [ln 2 / 2, ln 2);
    :428 wc = scale + 8 + 16 * decimation: the low nybble is 8 + scale."""
    ns = n_seg(bs)
    return {UNDEC} | {16 * (ns + seg) + 8 + sc for seg in range(ns) for sc in range(1, max_scale(bs) + 1)}


def position(wc):
    return (wc >> 4) & 15


def scale(wc):
    return wc & 7


def switched(wc):
    return wc != UNDEC


# ulcx_internal.h:171-179 ulcx_pattern (ulcHelper.h:24-46): per position digit the sub-blocks, first in the low nybble; bits 0-2
# of a nybble: the sub-block is BlockSize >> d, bit 3: the transient sub-block (its left overlap shrinks by the scale)
PATTERNS = [0x0000, 0x0008, 0x0019, 0x0091, 0x012A, 0x01A2, 0x02A1, 0x0A21, 0x123B, 0x12B3, 0x13B2, 0x1B32, 0x23B1, 0x2B31, 0x3B21, 0xB321]


def subblocks(wc, bs):
    """[(size, is the transient sub-block)] of a block"""
    p, out = PATTERNS[position(wc)], []
    while True:
        out.append((bs >> (p & 7), bool(p & 8)))
        p >>= 4
        if not p:
            return out


def first_overlap(wc, bs):
    """ulcx_enc_xf.hip:12-17: the left overlap a block asks for - its first sub-block's size, shrunk by the scale if that is the
    transient one."""
    size, transient = subblocks(wc, bs)[0]
    return size >> scale(wc) if transient else size


def overlaps(wc_prev, wc, wc_next, bs):
    """(ovFirst, nextOv) of xf_block, ulcx_enc_xf.hip:222-230: the block's left overlap clamped by the last sub-block of the
    block in front; the right overlap is what the block behind asks for (clamped per sub-block at :256)."""
    return min(first_overlap(wc, bs), subblocks(wc_prev, bs)[-1][0]), first_overlap(wc_next, bs)


def block_class(wc_prev, wc, wc_next, bs, k=2, pcm16=False):
    """Which form of the transform block k of a call takes (xf_block, ulcx_enc_xf.hip:219-256; xf_is_fast :187-201):
    ("steady",)            un-decimated, both overlaps full: at stereo 2048 / 4096 the all-constants path xf_fast
    ("steady_head",)       the same codes at block 0 or 1 of a PCM16 call: never xf_fast (:240, their history halves are float)
    ("left_cut",)          un-decimated, ovFirst < BlockSize: clamped by the last sub-block of the block in front
    ("right_cut",)         un-decimated, nextOv < BlockSize
    ("both_cut",)
    ("decimated", position, scale, switched in front, switched behind)"""
    ov_first, next_ov = overlaps(wc_prev, wc, wc_next, bs)
    if PATTERNS[position(wc)] >> 4:
        return ("decimated", position(wc), scale(wc), switched(wc_prev), switched(wc_next))
    left, right = ov_first < bs, next_ov < bs
    if left or right:
        return ("both_cut",) if left and right else ("left_cut",) if left else ("right_cut",)
    return ("steady_head",) if pcm16 and k < 2 else ("steady",)


def takes_xf_fast(cls, bs, ch):
    """ulcx_enc_xf.hip:240-241"""
    return cls == ("steady",) and ch == 2 and bs in (2048, 4096)


def clamp_kinds(wc_prev, wc, bs):
    """Two switched blocks in a row, by the order of their sub-block sizes at the seam: "front" - the last sub-block of the block
    in front is smaller than the overlap this block asks for, so both clamps fire: this block's ovFirst comes down to that
    sub-block (ulcx_enc_xf.hip:229) and so does the front block's nextOv (:255-256); "behind" - the overlap this block asks for
    is the smaller one and fits the front block's last sub-block, so nothing is clamped: both blocks lap over what this block
    asks for."""
    if not (switched(wc_prev) and switched(wc)):
        return set()
    last, ask = subblocks(wc_prev, bs)[-1][0], first_overlap(wc, bs)
    return ({"front"} if last < ask else set()) | ({"behind"} if ask < last else set())


UNDEC_CLASSES = [("steady",), ("left_cut",), ("right_cut",), ("both_cut",)]
NEIGHBOURS = [(False, False), (False, True), (True, False), (True, True)]      # a decimated block's (switched in front, behind)


def front_plan(K, wc_pipe, wc_steps=-1):
    """(transform cuts, window-control step boundaries) of a call of K blocks on an object whose plan reports wc_pipe chunks.
    ulcx_api.cpp enc_aux: the object's chunk count from 2 * wc_pipe blocks on, three chunks from 6 blocks, else the plain launch.
    ulcx_internal.h ulcx_front_plan: the first chunk is one block, the others cut the rest evenly; window control in four uniform
    steps from 8 blocks on, below that in the transform's chunks."""
    n_ch = wc_pipe if K >= 2 * wc_pipe else 3 if (K >= 6 and wc_pipe > 1) else 1
    if n_ch <= 1:
        return (0, K), (0, K)
    cut = [0, 1] + [1 + (K - 1) * (j - 1) // (n_ch - 1) for j in range(2, n_ch + 1)]
    n_w = wc_steps if wc_steps >= 0 else (4 if K >= 8 else 0)
    n_w = min(n_w, 32, K)
    steps = cut if n_w < 1 else [K * w // n_w for w in range(n_w + 1)]
    return tuple(cut), tuple(steps)


def boundaries(K, wc_pipe):
    """The interior boundaries of a call: {block index b: the kinds of boundary in front of block b}."""
    cut, steps = front_plan(K, wc_pipe)
    out = {}
    for kind, marks in (("cut", cut), ("step", steps)):
        for b in marks[1:-1]:
            out.setdefault(b, set()).add(kind)
    return out


# ---------------------------------------------------------------------------
# a designed input
# ---------------------------------------------------------------------------
BED = 2e-3                                              # standard deviation of the noise bed: about 65 PCM16 steps
POSITIONS = 16                                          # onsets across a block
GAINS = [10.0 ** (-1.6 + 0.3 * i) for i in range(14)]   # 14 levels over four decades, none of them 1
BURST, STEP = 0, 1                                      # shapes 2 .. 6: a linear onset of BlockSize >> (10, 8, 6, 4, 2) samples
SHAPES = (BURST, STEP, 2, 3, 4, 5, 6)
SPAN = 16                                               # the noise is laid out this many blocks to either side of the first event


def shape_name(shape):
    return "burst" if shape == BURST else "step" if shape == STEP else "ramp/%d" % (1 << (10 - 2 * (shape - 2)))


def designed(bs, ch, nblk, events, seed):
    """float32 [nblk * bs][ch] on the PCM16 grid: a Gaussian noise bed with one event per entry (block, pos, level, shape) of
    events.  The event's onset is sample block * bs - bs / 2 + pos * bs / 16: window control looks at a block through an envelope
    centred on the boundary between the block in front and this one, so the eight segments it compares for `block` begin half
    a block early.  burst: max(4, bs / 64) samples of noise GAINS[level] times the bed, added; step: the bed from there on times
    GAINS[level]; shapes 2 .. 6: the same gain reached over a linear onset.
    The noise is drawn relative to the first event, so moving that event to another block moves the signal with it.
    The samples are those of numpy's Generator.normal for these seeds, and TABLE below holds for exactly them: numpy does not
    promise the same stream in every version.  Should it change, the CPU census fails (a row no longer gives its code), and
    search() - python tests/window_axis_testlib.py - prints the table anew."""
    n = nblk * bs
    b0 = events[0][0]
    assert 0 <= b0 <= SPAN
    rng = np.random.default_rng([0x51A, bs, ch, seed])
    x = rng.normal(0.0, BED, (max(2 * SPAN, SPAN - b0 + nblk) * bs, ch))[(SPAN - b0) * bs:(SPAN - b0) * bs + n]     # (a longer draw begins with the shorter one)
    gain = np.ones(n)
    for j, (blk, pos, level, shape) in enumerate(events):
        t0 = blk * bs - bs // 2 + pos * bs // POSITIONS
        assert 0 <= t0 < n, (blk, pos)
        g = GAINS[level]
        if shape == BURST:
            ln = min(max(4, bs // 64), n - t0)
            x[t0:t0 + ln] += np.random.default_rng([0xB57, bs, ch, seed, j]).normal(0.0, BED * g, (ln, ch))
        else:
            ramp = 0 if shape == STEP else bs >> (10 - 2 * (shape - 2))
            ln = min(ramp, n - t0)
            gain[t0:t0 + ln] *= 1.0 + (g - 1.0) * (np.arange(ln) + 1) / (ramp + 1)
            gain[t0 + ln:] *= g
    x = x * gain[:, None]
    out = (np.clip(np.rint(x * 32768.0), -32768, 32767) * (1.0 / 32768.0)).astype(np.float32)
    out.setflags(write=False)
    return out


def oracle_wc(pcm, bs):
    """WindowCtrl of every block from the oracle's VBR 50 run"""
    return oracle_encode_stream(pcm, bs, RATE, quality=50.0)[2]


# ---------------------------------------------------------------------------
# the search (by hand; prints the TABLE below)
# ---------------------------------------------------------------------------
FIRST_EVENT_BLOCK = 2                                   # the blocks in front hold the stream's start


def trial_seed(pos, level, shape):
    return (shape * 100 + level) * 100 + pos


def search(geometries=GEOMETRIES, out=sys.stdout):
    """Walks the grid POSITIONS x GAINS x shapes with the oracle, one event per stream - the very stream code_stream() gives the
    tests - and prints per geometry one (code, pos, level, shape) per code seen in the two blocks behind the event's (a block's
    code is decided one block early, from the envelope of the block in front)."""
    for bs, ch in geometries:
        found = {}
        for shape in SHAPES:                            # (stops behind the first shape that completes the set)
            for level in range(len(GAINS)):
                for pos in range(POSITIONS):
                    e = code_event_block(pos, level, shape)
                    for c in oracle_wc(code_stream(bs, ch, pos, level, shape), bs)[e + 1:e + 3]:
                        if switched(int(c)):
                            found.setdefault(int(c), (pos, level, shape))
            if set(found) | {UNDEC} == codes(bs):
                break
        rows = ", ".join("(0x%02X, %d, %d, %d)" % ((c,) + found[c]) for c in sorted(found))
        print("    (%d, %d): [%s]," % (bs, ch, rows), file=out)
        missing = sorted(codes(bs) - set(found) - {UNDEC})
        print("    # %d x %d: %d of %d; not reached: %s" % (bs, ch, len(found) + 1, len(codes(bs)), " ".join("0x%02X" % c for c in missing) or "-"), file=out)
        out.flush()


# (geometry): [(code the oracle gave at the search, pos, level, shape)] - from search(), this project's oracle alone
TABLE = {
    (256, 2): [(0x49, 1, 10, 0), (0x59, 5, 10, 0), (0x69, 10, 10, 0), (0x79, 15, 10, 0)],
    (256, 1): [(0x49, 4, 9, 0), (0x59, 5, 10, 0), (0x69, 11, 11, 0), (0x79, 14, 10, 0)],
    (512, 3): [(0x89, 1, 9, 0), (0x99, 3, 10, 0), (0xA9, 5, 10, 0), (0xB9, 7, 10, 0), (0xC9, 9, 10, 0), (0xD9, 11, 10, 0), (0xE9, 13, 10, 0), (0xF9, 15, 8, 1)],
    (1024, 2): [(0x89, 1, 8, 0), (0x8A, 0, 9, 0), (0x99, 2, 8, 0), (0x9A, 3, 9, 0), (0xA9, 5, 8, 0), (0xAA, 5, 9, 0), (0xB9, 7, 0, 1), (0xBA, 7, 9, 0),
                (0xC9, 8, 8, 0), (0xCA, 10, 9, 0), (0xD9, 11, 1, 1), (0xDA, 11, 8, 0), (0xE9, 12, 0, 1), (0xEA, 13, 9, 0), (0xF9, 15, 0, 2), (0xFA, 15, 8, 0)],
    (2048, 2): [(0x89, 1, 3, 2), (0x8A, 0, 7, 0), (0x8B, 0, 8, 0), (0x99, 3, 7, 0), (0x9A, 2, 7, 0), (0x9B, 3, 8, 0), (0xA9, 4, 0, 2), (0xAA, 4, 7, 0),
                (0xAB, 5, 8, 0), (0xB9, 6, 4, 1), (0xBA, 6, 7, 0), (0xBB, 7, 7, 0), (0xC9, 8, 6, 0), (0xCA, 8, 7, 0), (0xCB, 9, 8, 0), (0xD9, 10, 6, 0),
                (0xDA, 10, 7, 0), (0xDB, 10, 8, 0), (0xE9, 14, 1, 1), (0xEA, 12, 7, 0), (0xEB, 13, 8, 0), (0xF9, 14, 6, 0), (0xFA, 15, 7, 0), (0xFB, 15, 8, 0)],
    (4096, 2): [(0x89, 10, 7, 0), (0x8A, 15, 10, 1), (0x8B, 0, 6, 0), (0x8C, 0, 7, 0), (0x99, 14, 7, 0), (0x9A, 2, 6, 0), (0x9B, 2, 7, 0), (0x9C, 3, 7, 0),
                (0xA9, 14, 9, 0), (0xAA, 4, 0, 1), (0xAB, 4, 6, 0), (0xAC, 5, 7, 0), (0xB9, 5, 1, 0), (0xBA, 6, 6, 0), (0xBB, 6, 7, 0), (0xBC, 7, 7, 0),
                (0xC9, 15, 10, 0), (0xCA, 8, 6, 0), (0xCB, 8, 7, 0), (0xCC, 9, 7, 0), (0xD9, 13, 0, 0), (0xDA, 10, 6, 0), (0xDB, 12, 0, 1), (0xDC, 11, 7, 0),
                (0xE9, 7, 1, 0), (0xEA, 12, 6, 0), (0xEB, 13, 6, 0), (0xEC, 13, 7, 0), (0xF9, 14, 5, 1), (0xFA, 14, 6, 0), (0xFB, 14, 7, 0), (0xFC, 15, 7, 0)],
    (2048, 1): [(0x89, 0, 7, 0), (0x8A, 1, 7, 0), (0x8B, 1, 8, 0), (0x99, 2, 7, 0), (0x9A, 2, 0, 1), (0x9B, 3, 8, 0), (0xA9, 4, 0, 1), (0xAA, 5, 7, 0),
                (0xAB, 5, 8, 0), (0xB9, 6, 7, 0), (0xBA, 7, 7, 0), (0xBB, 7, 8, 0), (0xC9, 8, 7, 0), (0xCA, 9, 0, 1), (0xCB, 9, 8, 0), (0xD9, 10, 1, 1),
                (0xDA, 10, 7, 0), (0xDB, 11, 8, 0), (0xE9, 13, 1, 1), (0xEA, 12, 7, 0), (0xEB, 12, 8, 0), (0xF9, 14, 1, 1), (0xFA, 14, 7, 0), (0xFB, 15, 8, 0)],
    (8192, 3): [(0x89, 0, 0, 0), (0x8A, 1, 5, 0), (0x8B, 11, 7, 0), (0x8C, 14, 6, 0), (0x8D, 0, 6, 0), (0x99, 14, 2, 0), (0x9A, 0, 5, 0), (0x9B, 15, 6, 0),
                (0x9C, 3, 6, 0), (0x9D, 3, 7, 0), (0xA9, 12, 0, 0), (0xAA, 2, 5, 0), (0xAB, 4, 6, 0), (0xAC, 2, 6, 0), (0xAD, 5, 7, 0), (0xB9, 9, 0, 0),
                (0xBA, 7, 5, 0), (0xBB, 4, 5, 1), (0xBC, 7, 6, 0), (0xBD, 7, 7, 0), (0xC9, 12, 2, 0), (0xCA, 5, 5, 1), (0xCB, 6, 6, 0), (0xCC, 6, 7, 0),
                (0xCD, 9, 6, 0), (0xD9, 8, 0, 0), (0xDA, 8, 5, 1), (0xDB, 8, 6, 0), (0xDC, 8, 7, 0), (0xDD, 11, 6, 0), (0xE9, 11, 0, 0), (0xEA, 8, 8, 0),
                (0xEB, 14, 0, 1), (0xEC, 10, 6, 0), (0xED, 13, 7, 0), (0xF9, 2, 0, 0), (0xFA, 2, 2, 0), (0xFB, 14, 6, 0), (0xFC, 12, 6, 0), (0xFD, 15, 7, 0)],
    (16384, 1): [(0x89, 2, 1, 0), (0x8A, 0, 5, 0), (0x8B, 13, 8, 0), (0x8C, 1, 6, 0), (0x8D, 12, 0, 1), (0x8E, 0, 7, 0), (0x99, 6, 2, 0), (0x9A, 1, 5, 1),
                 (0x9B, 0, 6, 0), (0x9C, 3, 6, 0), (0x9D, 2, 7, 1), (0x9E, 3, 7, 0), (0xA9, 9, 1, 0), (0xAA, 2, 5, 0), (0xAB, 4, 6, 1), (0xAC, 2, 6, 0),
                 (0xAD, 4, 7, 3), (0xAE, 2, 7, 0), (0xB9, 13, 0, 0), (0xBA, 6, 5, 0), (0xBB, 6, 6, 1), (0xBC, 4, 6, 0), (0xBD, 6, 7, 3), (0xBE, 4, 7, 0),
                 (0xC9, 0, 0, 0), (0xCA, 7, 5, 1), (0xCB, 8, 6, 1), (0xCC, 6, 6, 0), (0xCD, 9, 6, 0), (0xCE, 6, 7, 0), (0xD9, 8, 5, 0), (0xDA, 9, 5, 1),
                 (0xDB, 8, 6, 0), (0xDC, 11, 6, 1), (0xDD, 10, 7, 3), (0xDE, 8, 7, 0), (0xE9, 3, 0, 0), (0xEA, 13, 5, 0), (0xEB, 12, 6, 1), (0xEC, 10, 6, 0),
                 (0xED, 13, 6, 0), (0xEE, 10, 7, 0), (0xF9, 12, 0, 0), (0xFA, 1, 13, 0), (0xFB, 14, 6, 0), (0xFC, 12, 6, 0), (0xFD, 14, 7, 2), (0xFE, 12, 7, 0)],
    (32768, 1): [(0x89, 0, 3, 0), (0x8A, 13, 11, 0), (0x8B, 13, 12, 0), (0x8C, 14, 6, 0), (0x8D, 13, 13, 0), (0x8E, 14, 4, 2), (0x8F, 1, 7, 0), (0x99, 1, 5, 1),
                 (0x9A, 0, 5, 0), (0x9B, 3, 6, 1), (0x9C, 0, 4, 1), (0x9D, 0, 6, 0), (0x9E, 1, 4, 1), (0x9F, 0, 7, 0), (0xA9, 2, 5, 0), (0xAA, 5, 6, 1),
                 (0xAB, 4, 6, 1), (0xAC, 2, 6, 0), (0xAD, 3, 6, 0), (0xAE, 3, 4, 1), (0xAF, 2, 7, 0), (0xB9, 12, 5, 0), (0xBA, 5, 5, 2), (0xBB, 6, 6, 1),
                 (0xBC, 4, 6, 0), (0xBD, 4, 4, 1), (0xBE, 5, 4, 1), (0xBF, 4, 7, 0), (0xC9, 9, 4, 0), (0xCA, 7, 5, 3), (0xCB, 8, 6, 1), (0xCC, 6, 6, 0),
                 (0xCD, 6, 4, 3), (0xCE, 6, 4, 1), (0xCF, 6, 7, 0), (0xD9, 10, 5, 1), (0xDA, 9, 5, 0), (0xDB, 10, 6, 1), (0xDC, 8, 6, 0), (0xDD, 8, 4, 1),
                 (0xDE, 9, 4, 1), (0xDF, 8, 7, 0), (0xE9, 4, 3, 0), (0xEA, 13, 6, 5), (0xEB, 12, 6, 1), (0xEC, 10, 6, 0), (0xED, 10, 4, 1), (0xEE, 11, 4, 2),
                 (0xEF, 10, 7, 0), (0xF9, 14, 5, 0), (0xFA, 15, 1, 1), (0xFB, 14, 6, 0), (0xFC, 12, 6, 0), (0xFD, 14, 7, 2), (0xFE, 12, 4, 1), (0xFF, 12, 7, 0)],
}

# codes of codes(bs) the search did not reach, by name, with the grid that was tried (POSITIONS x GAINS x SHAPES): none - the search reached every code of every geometry
NOT_REACHED = {
}


# ---------------------------------------------------------------------------
# the cases: streams and their oracle runs, computed once per process, shared by every test, never written to
# ---------------------------------------------------------------------------
CODE_K, CODE_CALLS = 5, 2                               # a code case: two consecutive calls of 5 blocks
CODE_BLOCKS = CODE_K * CODE_CALLS


def code_event_block(pos, level, shape):
    """The block of a table row's event: 2 .. 7 - the switched block behind it is block 3 or 4 of the first call or 0 .. 3 of the
    second - by a rule that does not ask what the event does: a row's code holds for this block (the envelopes' memory makes
    the scale depend a little on how long the stream has run)."""
    return FIRST_EVENT_BLOCK + (pos + 3 * level + shape) % 6


def code_stream(bs, ch, pos, level, shape):
    return designed(bs, ch, CODE_BLOCKS, [(code_event_block(pos, level, shape), pos, level, shape)], trial_seed(pos, level, shape))


@functools.lru_cache(maxsize=None)
def code_streams(bs, ch):
    """[codes of the table][10 * bs][ch]: stream i holds the table's i-th event."""
    pcm = np.stack([code_stream(bs, ch, pos, level, shape) for _, pos, level, shape in TABLE[(bs, ch)]])
    pcm.setflags(write=False)
    return pcm


# Streams with events in two to four blocks in a row, each louder than the one in front (a burst masks what follows it for more
# than a block at the small sizes): early after early and late after late transients, so that the smaller sub-block at the seam is
# once the front block's last and once this block's first; early after late and late after early; an un-decimated block between two
# switched ones; steps instead of bursts.  [[(block, pos, level, shape)]], the same at every geometry.
NEIGHBOUR_EVENTS = [
    [(2, 0, 7, BURST), (3, 0, 10, BURST)], [(2, 15, 7, BURST), (3, 15, 10, BURST)], [(3, 0, 7, BURST), (4, 15, 10, BURST)], [(3, 15, 7, BURST), (4, 0, 10, BURST)],
    [(2, 8, 7, BURST), (4, 8, 10, BURST)], [(2, 0, 6, BURST), (3, 8, 9, BURST), (4, 15, 12, BURST)], [(4, 15, 6, BURST), (5, 0, 9, BURST), (6, 8, 12, BURST)],
    [(3, 4, 8, STEP), (4, 4, 8, STEP)], [(3, 12, 8, STEP), (4, 12, 8, STEP)],
    [(2, 2, 7, BURST), (3, 2, 9, BURST), (4, 2, 11, BURST), (5, 2, 13, BURST)], [(2, 13, 7, BURST), (3, 13, 9, BURST), (4, 13, 11, BURST), (5, 13, 13, BURST)],
    [(2, 4, 10, BURST)], [(2, 12, 10, BURST)],              # behind the switch of the stream's start: an un-decimated block between two switches
]
# What no stream reaches, by name.  BlockSize 256: two switched blocks in a row whose seam clamps ovFirst ("front": 0x69 or 0x79 behind
# 0x69 or 0x79).  Tried: the streams above, every pair of late onsets (pos 10 .. 15) in blocks 3 and 4 as bursts, steps and two
# onset shapes at eight level pairs, and 3000 streams of two or three random events (any pos, level, shape) in blocks in a row.
NO_CLAMP = {(256, 2): ("front",), (256, 1): ("front",)}


@functools.lru_cache(maxsize=None)
def neighbour_streams(bs, ch):
    pcm = np.stack([designed(bs, ch, CODE_BLOCKS, events, 7000 + i) for i, events in enumerate(NEIGHBOUR_EVENTS)])
    pcm.setflags(write=False)
    return pcm


POSITION_GEOMETRIES = [(2048, 2), (2048, 1)]            # fused k_wc_ef; split k_wc_energy + k_wc_forward
POSITION_KS = [5, 6, 7, 8, 9, 11]
WC_PIPE = 4                                             # what an object with side streams reports (ulcx_api.cpp:319)


def position_events(bs, ch, K):
    """2 K + 2 streams of two calls of K blocks: stream s < 2 K has a burst in block s % K of the first call and a louder one in
    block (s + 1) % K of the second (louder: the two may be neighbours, and a burst masks what follows it; block 0 of the first
    call holds the stream's start instead, an event's onset lies half a block in front), the onsets at different places of the
    block.  The last two have louder and louder bursts in blocks in a row up to the call boundary and across it, so that the code
    carried into the second call and the one in front of it are both switches."""
    out = []
    for s in range(2 * K):
        pos = (3 * s) % POSITIONS
        out.append([(b, pos, level, BURST) for b, level in ((s % K, 9), (K + (s + 1) % K, 12)) if b > 0])
    out.append([(K - 3, 2, 7, BURST), (K - 2, 2, 9, BURST), (K - 1, 2, 11, BURST)])
    out.append([(K - 3, 13, 7, BURST), (K - 2, 13, 9, BURST), (K - 1, 13, 11, BURST), (K, 13, 13, BURST)])
    return out


@functools.lru_cache(maxsize=None)
def position_streams(bs, ch, K):
    pcm = np.stack([designed(bs, ch, 2 * K, events, 9000 + 100 * K + s) for s, events in enumerate(position_events(bs, ch, K))])
    pcm.setflags(write=False)
    return pcm


@functools.lru_cache(maxsize=None)
def oracle_runs(kind, bs, ch, K=0):
    """The oracle's VBR 50 debug run (ulc_testlib.oracle_encode_debug) of every stream of code_streams / neighbour_streams /
    position_streams."""
    pcm = {"code": code_streams, "neighbour": neighbour_streams}[kind](bs, ch) if kind != "position" else position_streams(bs, ch, K)
    return tuple(oracle_encode_debug(x, bs, RATE, 0, 50.0) for x in pcm)


@functools.lru_cache(maxsize=None)
def oracle_decoded(kind, bs, ch):
    """(blocks uint8 [streams][blocks][slot], pcm float32, bits): the oracle's bytes of the streams and its own decode of them."""
    refs = oracle_runs(kind, bs, ch)
    blocks = np.stack([r["out"] for r in refs])
    pcm, bits = [], []
    for s, r in enumerate(refs):
        rc, p, b = oracle_decode_stream(r["out"], ch, bs)
        assert rc == 0, f"{bs} x {ch} stream {s}: the oracle refuses its own stream ({rc})"
        pcm.append(p); bits.append(b)
    return blocks, np.stack(pcm), np.stack(bits)


def wc_rows(refs):
    return [[int(v) for v in r["wc"]] for r in refs]


def classes_of(row, bs, K, pcm16=False):
    """block_class of every block of a stream run in calls of K blocks; the code in front of block 0 and behind the last one:
    0x10 in front (a fresh encoder's state), and the last block is left out (its successor is not known)."""
    out = []
    for k in range(len(row) - 1):
        out.append(block_class(row[k - 1] if k else UNDEC, row[k], row[k + 1], bs, k % K, pcm16))
    return out


if __name__ == "__main__":
    args = [tuple(int(v) for v in a.split("x")) for a in sys.argv[1:]]
    search(args or GEOMETRIES)
