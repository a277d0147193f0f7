"""Inputs and oracle references of the splice tests (tests/test_splice_capi.py, tests/test_gpu_splice.py): source corpora made of
the streams of seek_testlib.geometries(), the rule by which an output file takes its blocks (include/ulc_amd.h, "Corpus splice"),
and what the oracle says about the result - the expected payload is the numpy concatenation of the source blocks at the sizes
the oracle reports, the expected index seek_testlib.oracle_walk of that concatenation, the expected PCM seek_testlib.oracle_pcm of
the concatenated block rows.  Nothing here comes from the library.  CPU only."""
import functools
import numpy as np
from seek_testlib import SEED0, geometries, oracle_pcm, oracle_stream, oracle_walk
from corpus_testlib import INDEX_DTYPE, File, Corpus, geom_files

SEGMENT_DTYPE = np.dtype([("File", np.int32), ("First", np.int32), ("Count", np.int32)])
GEOMS = sorted(geometries())
STEREO = (2048, 2)
ROTATE = 7                                                 # a geometry with one stream: file 1 is its blocks from block 7 on, then blocks 0 .. 6
FOREIGN_STATE = 0xDEADBEEF                                 # every RngState of a source index: the call never reads one
SWITCH_Q = (50.0, 20.0)                                    # the two rungs of the rung-switch tests: VBR 50 and VBR 20 of one clip


def source_of(files, payloads=None, offs=None):
    """A source corpus in both layouts (corpus_testlib.Corpus).  payloads: what the buffers hold (a damaged copy of a file's
    payload under the clean file's index, for the damage tests); offs: the index the buffers hold (an untrusted one, for some
    tests); the index is the oracle's offsets with FOREIGN_STATE for every state, in rows with three entries to spare."""
    return Corpus(files, payloads=payloads, offs=offs, states=FOREIGN_STATE, index_slack=3)


def extent(src, f, k):
    """Bytes of block k of file f as the buffers hold them, under the index they hold."""
    return src.payloads[f][max(int(src.offs[f][k]), 0):max(int(src.offs[f][k + 1]), 0)]


def takes(src, f, k):
    """The two entries that bound block k of file f satisfy 0 <= ByteOffs[k] < ByteOffs[k + 1] <= the file's bytes, and the
    oracle's parse of that extent is valid and consumes exactly the extent."""
    ok = src.__dict__.setdefault("_takes", {})
    if (f, k) not in ok:
        o0, o1 = int(src.offs[f][k]), int(src.offs[f][k + 1])
        ok[(f, k)] = 0 <= o0 < o1 <= len(src.payloads[f])
        if ok[(f, k)]:
            e = extent(src, f, k)
            bits = oracle_walk(e, len(e), src.ch, src.bs, 1)[0]
            ok[(f, k)] = len(bits) == 1 and (int(bits[0]) + 7) // 8 == len(e)
    return ok[(f, k)]


def row(src, f, k):
    """The block as a row of the oracle's slot size (zeros behind its bytes)."""
    r = np.zeros(src.files[f].blocks.shape[1], np.uint8)
    e = extent(src, f, k)
    r[:len(e)] = e
    return r


@functools.lru_cache(maxsize=None)
def source(geom):
    files = list(geom_files(geom))
    if len(files) == 1:
        f = files[0]
        order = [(k + ROTATE) % f.K for k in range(f.K)]
        files.append(File(f.name + f", from block {ROTATE} on", f.bs, f.ch, f.blocks[order], f.bits[order]))
    return source_of(files[:2])


@functools.lru_cache(maxsize=None)
def switch_source():
    """One clip (the stereo 2048 stream of seek_testlib) under the two rungs -> (source of two files, wc of each)."""
    bs, ch = STEREO
    enc = [oracle_stream(bs, ch, q, 3) for q in SWITCH_Q]
    return source_of([File(f"rung VBR {q:g}", bs, ch, e[0], e[1]) for q, e in zip(SWITCH_Q, enc)]), [np.asarray(e[2]) for e in enc]


def alternate(K, every, n_rungs=2):
    """The segments of one output file that switches rung every `every` blocks: [(rung, first, count)] over blocks 0 .. K - 1."""
    return [((k // every) % n_rungs, k, min(every, K - k)) for k in range(0, K, every)]


# ---------------------------------------------------------------------------------------------------------------------
# the rule, and the oracle's answers
# ---------------------------------------------------------------------------------------------------------------------
def seg_arrays(files):
    """[[(file, first, count)]] -> (seg_offs int32 [nOut + 1], seg SEGMENT_DTYPE [nSeg >= 1])"""
    offs = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int32)
    flat = [g for f in files for g in f]
    seg = np.zeros(max(len(flat), 1), SEGMENT_DTYPE)
    if flat:
        seg[:len(flat)] = np.array([tuple(int(x) for x in g) for g in flat], SEGMENT_DTYPE)
    return offs, seg


def plan_starts(segs):
    """d_segStart of one output file: the sum of max(Count, 0) over the earlier segments, saturating at INT32_MAX."""
    out, at = [], 0
    for _, _, count in segs:
        out.append(min(at, 2 ** 31 - 1))
        at += max(int(count), 0)
    return out


def taken(src, segs, out_stride, out_istride, gone=()):
    """The blocks [(file, block)] output file `segs` takes: one by one, in order, up to the first that cannot be taken.
    gone: files whose offsets the ragged form does not accept - they do not exist."""
    got, nbytes = [], 0
    for f, first, count in segs:
        for r in range(max(int(count), 0)):
            k = first + r
            if not (0 <= f < src.F) or f in gone or first < 0 or k >= src.files[f].K or not takes(src, f, k):
                return got
            n = len(extent(src, f, k))
            if len(got) + 1 > out_istride - 1 or nbytes + n > out_stride:
                return got
            got.append((f, k)); nbytes += n
    return got


class Expected:
    """What the call must leave of one output file: payload bytes, the whole index row, counts - the oracle's walk of the
    concatenation - and the oracle's decode of the concatenated rows."""

    def __init__(self, src, blocks, out_istride):
        self.blocks = blocks
        ext = [extent(src, f, k) for f, k in blocks]
        self.payload = np.concatenate(ext).astype(np.uint8) if ext else np.zeros(0, np.uint8)
        self.nbytes, self.n = len(self.payload), len(blocks)
        self.max_block = max((len(e) for e in ext), default=0)
        bits, offs, seeds, inside = oracle_walk(self.payload, self.nbytes, src.ch, src.bs, out_istride - 1)
        assert inside and len(bits) == self.n and int(offs[-1]) == self.nbytes, "the oracle walks the concatenation block for block"
        self.bits = bits
        self.index = np.zeros(out_istride, INDEX_DTYPE)
        self.index["ByteOffs"] = -1
        self.index["ByteOffs"][:self.n + 1] = offs
        self.index["RngState"][:self.n + 1] = seeds
        assert self.index[0]["ByteOffs"] == 0 and self.index[0]["RngState"] == SEED0
        self._src = src

    @functools.cached_property
    def pcm(self):
        """[n][bs][ch]: the oracle's sequential decode of the taken blocks as a file of their own."""
        if not self.blocks:
            return np.zeros((0, self._src.bs, self._src.ch), np.float32)
        rows = np.stack([row(self._src, f, k) for f, k in self.blocks])
        pcm, bits = oracle_pcm(rows, self._src.ch, self._src.bs)
        assert np.array_equal(bits, self.bits)
        return pcm


def expected(src, files, out_stride, out_istride, cache=None, gone=()):
    """-> ([Expected per output file], seg_start int32 [nSeg]); cache: {key of (segments): Expected} shared between equal files."""
    cache = {} if cache is None else cache
    out, starts = [], []
    for segs in files:
        key = (tuple(tuple(int(x) for x in g) for g in segs), out_stride, out_istride, tuple(gone))
        if key not in cache:
            cache[key] = Expected(src, taken(src, segs, out_stride, out_istride, gone), out_istride)
        out.append(cache[key])
        starts += plan_starts(segs)
    return out, np.array(starts, np.int32).reshape(-1)


# ---------------------------------------------------------------------------------------------------------------------
# the shapes of a splice (test 1), the alignment pairs of the copy (test 6), more files than a grid (test 7)
# ---------------------------------------------------------------------------------------------------------------------
def shapes(src):
    """One call's output files, by name -> [(name, [(file, first, count)])]"""
    K0, K1 = src.files[0].K, src.files[1].K
    many = [(j & 1, (j // 2) % min(K0, K1), 1) for j in range(130)]
    return [
        ("identity", [(0, 0, K0)]),
        ("head trim", [(0, 5, K0 - 5)]),
        ("tail trim", [(0, 0, K0 - 9)]),
        ("middle range", [(1, 6, 11)]),
        ("two files joined", [(0, 0, K0), (1, 0, K1)]),
        ("one file twice", [(1, 0, K1), (1, 0, K1)]),
        ("file 0 again", [(0, 3, 4)]),
        ("file 0 once more", [(0, 0, 2), (0, K0 - 2, 2)]),
        ("zero-count segments between real ones", [(0, 4, 0), (0, 2, 3), (1, 9, 0), (0, 0, 0), (1, 1, 2), (0, 7, 0)]),
        ("empty", []),
        ("130 one-block segments", many),
        ("file 0 three times", [(0, 0, K0)] * 3),             # 3 x 40 blocks (3 x 24 of a hand-assembled stream): more than 64
    ]


@functools.lru_cache(maxsize=None)
def alignment_blocks(seed=5):
    """Blocks [(file, block)] of the two stereo 2048 files for ONE output file in which every pair (source start mod 16, destination
    start mod 16) occurs: greedy - at every step the first block, in a seeded order, whose pair is new; when none is, the block that
    moves the destination to the residue with the most pairs still open."""
    src = source(STEREO)
    rng = np.random.default_rng(seed)
    cand = [(f, k) for f in range(2) for k in range(src.files[f].K)]
    cand = [cand[i] for i in rng.permutation(len(cand))]
    seen, out, at = set(), [], 0
    while len(seen) < 256 and len(out) < 2000:
        pick = next((c for c in cand if (int(src.files[c[0]].offs[c[1]]) % 16, at % 16) not in seen), None)
        if pick is None:
            open_at = lambda d: sum((s, d) not in seen for s in range(16))
            pick = max(cand, key=lambda c: open_at((at + int(src.files[c[0]].nb[c[1]])) % 16))
        seen.add((int(src.files[pick[0]].offs[pick[1]]) % 16, at % 16))
        out.append(pick)
        at += int(src.files[pick[0]].nb[pick[1]])
    return out


def alignment_pairs(blocks):
    src, seen, at = source(STEREO), set(), 0
    for f, k in blocks:
        seen.add((int(src.files[f].offs[k]) % 16, at % 16))
        at += int(src.files[f].nb[k])
    return seen, at


MANY_FILES = 16389
MANY_GEOM = (512, 1)


@functools.lru_cache(maxsize=None)
def many_patterns():
    """24 distinct one-segment files of 1 to 3 blocks of the 512 x 1 stream, and which of them each of the 16 389 output files is."""
    K = source(MANY_GEOM).files[0].K
    pats = [(f, (5 * i + f) % (K - 3), 1 + i % 3) for i in range(12) for f in range(2)]
    assert len(set(pats)) == 24
    which = np.random.default_rng(3).integers(0, len(pats), MANY_FILES)
    return pats, which
